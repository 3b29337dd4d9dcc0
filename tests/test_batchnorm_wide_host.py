"""Host side of csrc/bn_wide.hip (no GPU): the plan option ``bn_wide`` and its 'auto' rule, the slab
rule against the workspace formula, and the exported symbols."""
import pytest


class _Plan(object):
    def __init__(self, value):
        self.opt = {'bn_wide': value}


def test_option_and_auto_rule_on_both_sides_of_the_threshold(monkeypatch):
    from elektronn2_amd.neuromancer import neural, options, plan_options
    assert options.SPEC['bn_wide'][0] == 'E2_BN_WIDE' and options.get('bn_wide') == 'auto'
    for text, value in (('auto', 'auto'), ('1', True), ('0', False)):
        monkeypatch.setenv('E2_BN_WIDE', text)
        assert options.get('bn_wide') == value
    with plan_options(bn_wide=True):
        assert options.snapshot()['bn_wide'] is True                       # (what a Plan keeps)
    node = object.__new__(neural.Conv)
    T = node.BN_WIDE_MIN_COUNT
    assert T > 20 * 24 * 24                                                # config 1's largest channel
    below, at = (1, 7, 1, 1, T - 1), (1, 7, 1, 1, T)
    assert not node._bn_wide(_Plan('auto'), below) and node._bn_wide(_Plan('auto'), at)
    assert node._bn_wide(_Plan('auto'), (2, 32, 4, T // 16, 2))            # batch and every spatial axis count
    assert node._bn_wide(_Plan(True), below) is True and node._bn_wide(_Plan(False), at) is False
    with pytest.raises(ValueError, match="bn_wide"):
        node._bn_wide(_Plan('yes'), at)


@pytest.mark.parametrize("shape", [(1, 32, 116, 132, 132), (1, 200, 23, 90, 90), (2, 3, 3, 17, 19),
                                   (1, 4, 1, 1, 257), (20, 12, 1, 12, 12), (1, 1, 1, 1, 1)], ids=str)
def test_slabs_cover_the_rows_and_the_workspace_is_what_the_two_calls_need(shape):
    from elektronn2_amd.backend import Context, E2Error
    n, C, d, h, w = shape
    rows = n * d * h
    for splits in (0, 1, 3, rows):
        if splits > min(rows, 1024):
            continue
        c = Context.batchnorm_wide_choice(shape, splits)
        G = c['slabs']
        assert c['limit'] == min(rows, 1024) and 1 <= G <= c['limit'] and c['work_groups'] == C * G
        assert G == splits or splits == 0
        assert G * (c['rows'] - 1) < rows <= G * c['rows']                 # covered, no empty slab
        if splits == 0:     # the library's: at most 64 slabs, none below 8192 elements, about 4 x 256 work-groups
            assert G <= 64 and (G == 1 or rows * w // G >= 8192) and C * (G - 1) < 1024
        # forward: 8 floats per slab + the channel's mean and std; backward: 2 floats per slab
        assert Context.batchnorm_wide_workspace_bytes(shape, splits) == 4 * max(8 * C * G + 2 * C, 2 * C * G)
    with pytest.raises(E2Error, match="e2_batchnorm_wide_choice"):
        Context.batchnorm_wide_choice(shape, min(rows, 1024) + 1)


def test_symbols_are_exported():
    from elektronn2_amd import backend
    for name in ('workspace_bytes', 'choice', 'fwd', 'bwd'):
        assert 'e2_batchnorm_wide_' + name in backend.EXPORTED_SYMBOLS
