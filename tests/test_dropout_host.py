"""Dropout, host side (no GPU): the NumPy restatement of the gate contract of include/e2hip.h
(Philox4x32-10) against the Random123 known answers; the ``dropout_rate`` parameter of
Conv / UpConv / Perceptron (neural.py:246-249); ``Model.dropout_rates`` (model.py:365-396); the
save -> modelload round trip; the per-rank stream offsets of the data-parallel step.

tests/test_dropout_gpu.py imports ``philox4x32_10`` and ``restated_gate`` from here: they are the
reference of every comparison there, never the kernels."""
import numpy as np
import pytest

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LO = np.uint64(0xffffffff)
S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al. 2011).  ctr: four uint32 values or arrays, key: two ints.
    Returns the four output words as uint64 arrays holding 32-bit values."""
    c = [np.asarray(v, dtype=np.uint64) & LO for v in ctr]
    k0, k1 = int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                 # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & LO, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & LO]
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return c


def restated_gate(n, rate, seed, counter, stream):
    """(keep[n] bool, scale float32) of the gate indices j = 0 .. n-1 -- include/e2hip.h:
    word = philox(ctr = (lo32(j >> 2), hi32(j >> 2), stream, counter), key = (lo32(seed),
    hi32(seed)))[j & 3]; T = rate >= 1 ? 0xffffffff : (uint32)(rate * 2^32); keep = word >= T;
    scale = 1 / (1 - rate), all in float32."""
    j = np.arange(int(n), dtype=np.uint64)
    q = j >> np.uint64(2)
    z = np.zeros_like(q)
    words = np.stack(philox4x32_10((q & LO, q >> S32, z + np.uint64(int(stream) & 0xffffffff),
                                    z + np.uint64(int(counter) & 0xffffffff)),
                                   (int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff)))
    word = words[(j & np.uint64(3)).astype(np.int64), np.arange(int(n))]
    rate = np.float32(rate)
    T = 0xffffffff if rate >= 1 else int(np.float32(rate * np.float32(4294967296.0)))
    return word >= np.uint64(T), np.float32(1.0) / (np.float32(1.0) - rate)


def threshold_fraction(rate):
    """1 - T / 2^32: the exact keep probability of the contract for a float32 rate"""
    rate = np.float32(rate)
    T = 0xffffffff if rate >= 1 else int(np.float32(rate * np.float32(4294967296.0)))
    return 1.0 - T / 4294967296.0


@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_numpy_philox_reproduces_the_random123_known_answers(ctr, key, out):
    got = tuple(int(v) for v in philox4x32_10(ctr, key))
    assert got == out, [hex(v) for v in got]


def test_restated_gate_is_a_function_of_the_index_alone():
    """vectorised = element by element; another counter / stream / seed is another gate; rate 0
    keeps everything with scale exactly 1"""
    keep, scale = restated_gate(1000, 0.5, 1234, 7, 3)
    for j in (0, 1, 5, 999):
        w = philox4x32_10((j >> 2, 0, 3, 7), (1234, 0))[j & 3]
        assert bool(keep[j]) == (int(w) >= 0x80000000)
    assert scale == np.float32(2.0)
    assert np.array_equal(keep[:400], restated_gate(400, 0.5, 1234, 7, 3)[0])
    for other in ((1234, 8, 3), (1234, 7, 4), (1235, 7, 3), (1234 + (1 << 32), 7, 3)):
        assert not np.array_equal(keep, restated_gate(1000, 0.5, *other)[0])
    k0, s0 = restated_gate(64, 0.0, 1, 2, 3)
    assert k0.all() and s0 == np.float32(1.0)
    # the kept fraction of the restated gate itself (the issue's own check: 0.4 and 1.1 sigma)
    n = 1 << 22
    for r in (0.1, 0.5):
        frac = restated_gate(n, r, 1234, 7, 3)[0].mean()
        assert abs(frac - threshold_fraction(r)) < 5 * np.sqrt(r * (1 - r) / n)


def _three_nodes():
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    inp = nm.Input((2, 1, 6, 24, 24), 'b,f,z,x,y', name='raw')
    c0 = nm.Conv(inp, 4, (1, 3, 3), (1, 2, 2), dropout_rate=0.3, name='c0')
    c1 = nm.Conv(c0, 4, (1, 3, 3), name='c1')                       # rate 0: no parameter
    up = nm.UpConv(c1, 3, (1, 2, 2), dropout_rate=0.25, name='up')
    return nm, inp, c0, c1, up


def test_nodes_own_a_nontrainable_rate_parameter():
    """neural.py:246-249: a (1,) non-trainable, unregularised parameter named dropout_rate in
    node.params, only for a non-zero rate; rates outside [0, 1) are refused"""
    nm, inp, c0, c1, up = _three_nodes()
    nm.model_manager.reset()
    x2 = nm.Input((3, 7), 'b,f', name='x2')
    pc = nm.Perceptron(x2, 5, dropout_rate=0.3, name='pc')
    p0 = nm.Perceptron(x2, 5, name='p0')
    for node, r in ((c0, 0.3), (up, 0.25), (pc, 0.3)):
        p = node.params['dropout_rate']
        assert p is node.dropout_rate
        assert p.get_value().shape == (1,) and p.get_value().dtype == np.float32
        assert p.get_value()[0] == np.float32(r)
        assert p.apply_train is False and not p.apply_reg
    for node in (c1, p0):
        assert node.dropout_rate is None and 'dropout_rate' not in node.params
    assert not c0._drop_per_feature and not up._drop_per_feature and pc._drop_per_feature
    for bad in (1.0, 1.5, -0.1):
        with pytest.raises(ValueError):
            nm.Conv(inp, 2, (1, 3, 3), dropout_rate=bad)
        with pytest.raises(ValueError):
            nm.UpConv(inp, 2, (1, 2, 2), dropout_rate=bad)
        with pytest.raises(ValueError):
            nm.Perceptron(x2, 2, dropout_rate=bad)


def test_model_dropout_rates_protocol():
    """model.py:365-396: getter in node order; setter takes a number (all nodes) or a sequence
    (node order); a net without dropout has an empty array -- and the attribute exists"""
    nm, inp, c0, c1, up = _three_nodes()
    m = c0._model
    assert [n.name for n in m.dropout_nodes()] == ['c0', 'up']
    r = m.dropout_rates
    assert isinstance(r, np.ndarray) and np.allclose(r.ravel(), [0.3, 0.25])
    m.dropout_rates = 0
    assert np.array_equal(m.dropout_rates.ravel(), [0, 0])
    assert 'dropout_rate' in c0.params                 # (switched off, not removed)
    m.dropout_rates = [0.5, 0.125]
    assert np.array_equal(m.dropout_rates.ravel(), np.float32([0.5, 0.125]))
    assert c0.dropout_rate.get_value()[0] == np.float32(0.5)
    m.dropout_rates = np.array([0.3, 0.25])
    m.dropout_rates = r                                # what the getter returned goes back in
    assert np.allclose(m.dropout_rates.ravel(), [0.3, 0.25])
    for bad in (1.0, -0.5, [0.1, 1.0]):
        with pytest.raises(ValueError):
            m.dropout_rates = bad
    assert np.allclose(m.dropout_rates.ravel(), [0.3, 0.25])     # a refused value changes nothing
    # the trainer's "rates to 0, validate, restore" on a net WITHOUT dropout
    from elektronn2_amd import nets
    nm.model_manager.reset()
    plain = nets.neuro3d_lite((None, 1, 7, 47, 47))
    rates = plain.dropout_rates
    assert isinstance(rates, np.ndarray) and rates.size == 0
    plain.dropout_rates = 0.0
    plain.dropout_rates = rates


def test_seed_and_counter_on_the_host():
    nm, inp, c0, c1, up = _three_nodes()
    m = c0._model
    st = m.dropout_state()
    assert st['counter'] == 0 and st['seed'] > 1500000000        # the wall clock, as the reference
    m.set_dropout_seed(1234)
    assert m.dropout_state() == dict(seed=1234, counter=0)
    m.set_dropout_seed((1 << 40) + 5, counter=9)
    assert m.dropout_state() == dict(seed=(1 << 40) + 5, counter=9)


def _dropout_net(sp=(7, 47, 47)):
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    inp = nm.Input((None, 1) + tuple(sp), 'b,f,z,x,y', name='raw')
    out = nm.Conv(inp, 6, (1, 4, 4), (1, 2, 2), dropout_rate=0.2)
    out = nm.Conv(out, 8, (3, 3, 3), (1, 2, 2))
    out = nm.Conv(out, 8, (1, 3, 3), dropout_rate=0.4)
    out = nm.Conv(out, 2, (1, 1, 1), activation_func='lin', dropout_rate=0.1)
    probs = nm.Softmax(out)
    target = nm.Input_like(probs, override_f=1, name='target')
    loss = nm.AggregateLoss(nm.MultinoulliNLL(probs, target, target_is_sparse=True), name='loss')
    model = nm.model_manager.getmodel()
    model.designate_nodes(input_node=inp, target_node=target, loss_node=loss, prediction_node=probs)
    return model


def test_save_and_modelload_keep_the_rates(tmp_path):
    """the host-only round trip of tests/test_checkpoint.py: descriptor kwargs + the parameter
    value; a rate changed after construction is the one that comes back; another patch size
    keeps the rates; seed and counter are not part of the file"""
    from elektronn2_amd.neuromancer.model import modelload, params_from_model_file
    m = _dropout_net()
    m.dropout_rates = [0.25, 0.4, 0.5]
    m.set_dropout_seed(77, counter=3)
    f = str(tmp_path / "drop.mdl")
    m.save(f)
    assert params_from_model_file(f)['conv']['dropout_rate'].shape == (1,)
    m2 = modelload(f, name='rebuilt')
    assert [n.name for n in m2.dropout_nodes()] == [n.name for n in m.dropout_nodes()]
    assert np.array_equal(m2.dropout_rates, m.dropout_rates)
    assert np.array_equal(m2.dropout_rates.ravel(), np.float32([0.25, 0.4, 0.5]))
    assert 'dropout_rate' not in m2.nodes['conv1'].params
    assert m2.dropout_state()['seed'] != 77 and m2.dropout_state()['counter'] == 0
    m3 = modelload(f, name='bigger', imposed_patch_size=(9, 60, 58), imposed_batch_size=2)
    assert m3.input_node.shape.shape == [2, 1, 9, 59, 55]
    assert np.array_equal(m3.dropout_rates, m.dropout_rates)
    # into an already constructed graph
    m4 = _dropout_net()
    modelload(f, m4)
    assert np.array_equal(m4.dropout_rates, m.dropout_rates)


def test_ranks_draw_from_distinct_streams():
    """parallel.dropout_stream: ordinal + (rank << 16) -- distinct for every (node, rank) pair"""
    from elektronn2_amd import parallel
    assert parallel.dropout_stream(0) == 0 and parallel.dropout_stream(5, 0) == 5
    seen = set(parallel.dropout_stream(o, r) for o in range(40) for r in range(16))
    assert len(seen) == 40 * 16
    assert parallel.dropout_stream(3, 2) == (2 << 16) + 3
    with pytest.raises(ValueError):
        parallel.dropout_stream(1 << 16, 0)
    a = restated_gate(4096, 0.5, 9, 0, parallel.dropout_stream(1, 0))[0]
    b = restated_gate(4096, 0.5, 9, 0, parallel.dropout_stream(1, 1))[0]
    assert 0.4 < (a != b).mean() < 0.6
