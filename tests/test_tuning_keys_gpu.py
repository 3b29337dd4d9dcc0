"""The tuning key a conv GEMM launch runs under is the key every lookup asks for.

Conv._sig_fwd / _sig_dgrad / _sig_wgrad and UpConv._tune_sigs are what Plan._refine_pack_rows,
Plan.side_forced and bf16_ahead.prepare look tilings up with; a launch that ran under another key
would still run and tune, and the lookups would silently miss (weight images keep worst-case rows,
bf16 operands are no longer made ahead, the side-stream flag is lost).  Here: one eager gradient
evaluation with autotune.launch_log on, and the multiset of logged keys is the multiset built from
the nodes; then the second call's _refine_pack_rows finds the tilings the table holds."""
import collections
import json

import numpy as np
import pytest

from oracle import e2_oracle as O
from test_model_gpu import CASES, build, table_entries

pytestmark = pytest.mark.gpu


def route(node, plan):
    """head, first and tail in the precedence of Conv._plan_alloc / _plan_fwd / _plan_bwd"""
    if node._fused_head(plan) is not None:
        return 'head'
    if node._fused_first(plan):
        return 'first'
    if node._tail(plan) is not None:
        return 'tail'
    return 'gemm'


def key(plan, kind, sig):
    suffix = "_bf16" if getattr(plan.ctx, 'mfma_dtype', 'f32') == 'bf16' else ""
    return "%s%s|%s" % (kind, suffix, ",".join(str(int(v)) for v in sig))


def expected_keys(plan):
    from elektronn2_amd import neuromancer as nm
    want, routes = [], collections.Counter()
    for n in plan.nodes:
        if type(n) is nm.UpConv:
            # (the data-gradient GEMM where the parent needs a gradient: it does in every net here)
            assert plan.needs_grad(n.parent)
            sigs = n._tune_sigs(plan)
            want += [key(plan, 'igemm', sigs['fwd'][0]), key(plan, 'igemm', sigs['dgrad'][0]),
                     key(plan, 'wgrad', sigs['wgrad'][0])]
            routes['upconv'] += 1
        elif type(n) is nm.Conv:
            r = route(n, plan)
            routes[r] += 1
            if r == 'gemm':
                want.append(key(plan, 'igemm', n._sig_fwd(plan)))
            if r not in ('head', 'first'):
                want.append(key(plan, 'wgrad', n._sig_wgrad(plan)))
            if r == 'gemm' and plan.needs_grad(n.parent):
                want.append(key(plan, 'igemm', n._sig_dgrad(plan)))
    return want, routes


def lite(sp=(7, 47, 47)):
    name, spec, sp_ = CASES[0]
    assert sp_ == sp
    rng = np.random.RandomState(0)
    x = rng.rand(1, 1, *sp).astype(np.float32)
    t = rng.randint(0, 2, (1, 1) + O.net_out_shape(spec, sp)).astype(np.float32)
    return build(name, sp, O.init_net(spec, 1, seed=1)), x, t


def finish(inp, last):
    """(1,1,1) 'lin' head on ``last``, Softmax, NLL"""
    from elektronn2_amd import neuromancer as nm
    out = nm.Conv(last, 2, (1, 1, 1), activation_func='lin')
    probs = nm.Softmax(out)
    target = nm.Input_like(probs, override_f=1, name='target')
    loss = nm.AggregateLoss(nm.MultinoulliNLL(probs, target, target_is_sparse=True), name='loss')
    model = nm.model_manager.getmodel()
    model.designate_nodes(input_node=inp, target_node=target, loss_node=loss, prediction_node=probs)
    rng = np.random.RandomState(4)
    x = rng.rand(*inp.shape.shape).astype(np.float32)
    t = rng.randint(0, 2, [1, 1] + probs.shape.spatial_shape).astype(np.float32)
    return model, x, t


def unet_like():
    """the net of test_model_gpu.test_unet_like_merge_parity"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(3)
    inp = nm.Input((1, 1, 12, 36, 36), 'b,f,z,x,y', name='raw')
    c0 = nm.Conv(inp, 8, (1, 3, 3))
    c1 = nm.Conv(c0, 8, (1, 3, 3))
    p1 = nm.Pool(c1, (1, 2, 2))
    c2 = nm.Conv(p1, 16, (3, 3, 3))
    c3 = nm.Conv(c2, 16, (3, 3, 3))
    mrg = nm.UpConvMerge(c1, c3, 24)
    c4 = nm.Conv(mrg, 8, (1, 3, 3))
    return finish(inp, c4)


def chain(modes=('same', 'valid')):
    """'same' conv on the input, 'valid' tanh conv, head: the framed input, the activation pair's dy
    (the first conv runs the fused first-layer kernels on its framed input)"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(5)
    inp = nm.Input((1, 1, 6, 20, 20), 'b,f,z,x,y', name='raw')
    c0 = nm.Conv(inp, 8, (1, 3, 3), conv_mode=modes[0])
    c1 = nm.Conv(c0, 8, (3, 3, 3), conv_mode=modes[1], activation_func='tanh')
    return finish(inp, c1)


def chain_same_inside():
    """... with the modes swapped: the GEMM launches of the 'same' conv read the framed output of
    the layer before, its data gradient the inset of the padded gradient (Conv._dy_inset)"""
    return chain(('valid', 'same'))


NETS = [('lite', lite, {}, {'first', 'gemm', 'tail', 'head'}),
        ('unet_like', unet_like, {}, {'gemm', 'head', 'upconv'}),
        ('chain', chain, {}, {'gemm', 'head'}),
        ('chain_same_inside', chain_same_inside, {}, {'gemm', 'head'}),
        ('lite_fuse_actbwd', lite, dict(fuse_actbwd=1), {'first', 'gemm', 'head'})]


@pytest.mark.parametrize("name,make,opts,must_route", NETS, ids=[n[0] for n in NETS])
def test_launch_keys_are_the_lookup_keys(name, make, opts, must_route, monkeypatch, tmp_path):
    from elektronn2_amd import autotune
    from elektronn2_amd.neuromancer import plan_options
    monkeypatch.setenv("E2HIP_AUTOTUNE", "0")          # nothing is timed
    with plan_options(**opts):
        model, x, t = make()
        autotune.launch_log = log = []
        try:
            model.gradients(x, t)                      # eager
        finally:
            autotune.launch_log = None
        plan = model._grad_func.func
        want, routes = expected_keys(plan)
        print(name, dict(routes), len(log), "launches")
        assert must_route <= set(routes), routes
        got = collections.Counter(k for k, _, _ in log)
        assert got == collections.Counter(want), (sorted((got - collections.Counter(want)).items()),
                                                  sorted((collections.Counter(want) - got).items()))
        if opts.get('fuse_actbwd'):
            assert any(isinstance(k, tuple) and len(k) == 2 and k[1] == 'dy_done' for k in plan.scratch)
        # the second call re-packs the weight images with the rows each launch's tiling reaches:
        # pin, for two launches that read an image, the 16x16x4 tiling the library ran them with
        imgs = {}            # key -> (node, mode) of the image its launch reads
        for node, md in plan.pack_nodes.values():
            if md == 0:
                imgs[key(plan, 'igemm', node._sig_fwd(plan))] = (node, md)
            elif plan.needs_grad(node.parent):
                imgs[key(plan, 'igemm', node._sig_dgrad(plan))] = (node, md)
        assert imgs and set(imgs) <= set(want)
        ran = {k: ll[1] for k, _, ll in log
               if k in imgs and ll is not None and ll[0] == 'igemm' and ll[1].count(",") == 3}
        pins = {}
        for k in sorted(imgs)[:2]:
            # (where the library chose another kernel family: the first 16x16x4 string without
            # split-K that the tuner would try on this very problem)
            s = [int(v) for v in k.split("|")[1].split(",")]
            cands = [c for c in autotune.igemm_candidates(s[1], s[2], tuple(s[3:6]), tuple(s[6:9]),
                                                          split_k=False) if c.count(",") == 3]
            pins[k] = ran.get(k) or cands[0]
        print(name, "pins", pins)
        assert len(pins) == 2
        fixture = tmp_path / "pins.json"
        fixture.write_text(json.dumps(pins))
        with table_entries(str(fixture)):
            model.gradients(x, t)
            known = {k: autotune.known(plan.ctx, 'igemm', k.split("|")[1].split(",")) for k in imgs}
        assert all(known[k] == v for k, v in pins.items())
        n_own = 0
        for k, (node, md) in imgs.items():
            wp = plan.scratch[node, 'wp_f' if md == 0 else 'wp_d']
            v = (known[k] or "").split(",")
            own = len(v) == 4 or (len(v) in (3, 5) and v[0] == '1')      # 16x16x4 / pointwise
            assert (id(wp) in plan._img_stride) == own, (k, known[k])
            n_own += own
        assert n_own >= 2 and len(plan._img_stride) == n_own
