"""Host side of csrc/dense_gemm.hip (no GPU): the plan option ``dense_gemm`` and its 'auto' rule on
built nodes, the split rule against the workspace formula, and the net the GPU file trains."""
import numpy as np
import pytest

from test_batchnorm_host import BnRef, _finish_nll, _nm, feed_for


def net_a():
    """(32, 600) -> Perceptron(256, relu) -> Perceptron(10, lin) -> Softmax -> NLL: the hidden layer
    above the 'auto' threshold, the head below"""
    nm = _nm(61)
    inp = nm.Input((32, 600), 'b,f', name='raw')
    out = nm.Perceptron(nm.Perceptron(inp, 256, name='hidden'), 10, activation_func='lin', name='head')
    return _finish_nll(nm, inp, out)


def test_auto_rule_and_the_three_values_on_built_nodes(monkeypatch):
    from elektronn2_amd.neuromancer import options, plan_options
    m = net_a()
    hidden, head = m.nodes['hidden'], m.nodes['head']
    assert hidden.DENSE_GEMM_MIN_MACS == 2 ** 22 > 20 * 576 * 200         # config 1's largest dot
    assert hidden.dense_gemm_route(32) and not head.dense_gemm_route(32)
    assert not hidden.dense_gemm_route(27) and hidden.dense_gemm_route(28)      # 27.3 * 600 * 256 = 2^22
    # the weight gradient: from the smallest measured shape at which it won, 128 * 784 * 512
    assert hidden.dense_gemm_route(32, 'auto', 'dgrad') and not hidden.dense_gemm_route(32, 'auto', 'wgrad')
    assert not hidden.dense_gemm_route(334, 'auto', 'wgrad') and hidden.dense_gemm_route(335, 'auto', 'wgrad')
    assert head.dense_gemm_route(1, True, 'wgrad') is True and hidden.dense_gemm_route(10 ** 6, False) is False
    with pytest.raises(ValueError, match="dense_gemm"):
        head.dense_gemm_route(32, 'yes')
    assert options.SPEC['dense_gemm'][0] == 'E2_DENSE_GEMM' and options.get('dense_gemm') == 'auto'
    for text, value in (('auto', 'auto'), ('1', True), ('0', False)):
        monkeypatch.setenv('E2_DENSE_GEMM', text)
        assert options.get('dense_gemm') == value
    with plan_options(dense_gemm=True):
        assert options.snapshot()['dense_gemm'] is True                    # (what a Plan keeps)
    # the reference steps of the GPU test are well-posed (no relu unit at its kink)
    ref = BnRef(m)
    feed = feed_for(m, 7, 10)
    assert all(np.isfinite(ref.step(feed, 'SGD')) for _ in range(2))


@pytest.mark.parametrize("n,k,m", [(128, 784, 512), (32, 20000, 256), (32, 600, 256), (20, 576, 200), (1, 3, 1)])
def test_workspace_is_the_largest_slab_stack_of_the_split_rule(n, k, m):
    from elektronn2_amd.backend import Context
    dims = dict(fwd=(n, m, k), dgrad=(n, k, m), wgrad=(k, m, n))           # M, N, K
    for splits in (0, 1, 3):
        need = 0
        for op, (M, N, K) in dims.items():
            c = Context.dense_gemm_choice(op, n, k, m, min(splits, -(-K // 4)))
            assert c['tile'] == ((16, 128) if M <= 32 else (64, 64))
            assert c['tiles'] == -(-M // c['tile'][0]) * -(-N // c['tile'][1])
            assert 1 <= c['splits'] <= c['limit'] == min(-(-K // 4), 1024)
            # every k is dealt out, and the last split is not empty
            assert 4 * c['per'] * (c['splits'] - 1) < K <= 4 * c['per'] * c['splits']
            if splits == 0 and c['splits'] > 1:     # the library's: whole chunks, no split of a full grid
                assert c['per'] % 8 == 0 and c['per'] >= 16 and c['splits'] <= 64 and 4 * c['tiles'] <= 256
            need = max(need, 4 * c['splits'] * M * N if c['splits'] > 1 else 0)
        assert Context.dense_gemm_workspace_bytes(n, k, m, splits) == need
