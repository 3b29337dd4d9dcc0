"""Host-side switches of the launch plan as ARGUMENTS.

Until round 4 the plan read ``E2_*`` environment variables at import, at build and per step, and
a test flipped ``os.environ`` mid-process to choose a code path.  Now every switch is a named
option: ``set_plan_options(name=value, ...)`` changes the process-wide default, ``plan_options(
name=value, ...)`` is the same as a context manager, and a ``Plan`` SNAPSHOTS the options when
it is constructed (``Plan.opt``) -- a plan never changes behaviour after it was built or
captured, whatever is set later.  The environment variable of each option is its DEFAULT only
(read when the option is first asked for), kept so that the A/B scripts under tools/ still work.

The reference has no counterpart (Theano's flags, ``theano.config.*``, are the closest analogue:
process-wide, read at compile time -- graphutils.py:376-387)."""
import contextlib
import os


def _b(v):
    return str(v).strip().lower() not in ("0", "", "false", "off", "no")


def _tri(v):
    return None if v is None or str(v) == "" else _b(v)


# name: (environment variable, parser, default, what it does)
SPEC = {
    "graph": ("E2_NO_GRAPH", lambda v: not _b(v), True,
              "capture the step into hipGraphs after one eager call (E2_NO_GRAPH=1 turns it off)"),
    "side_stream": ("E2_SIDE_STREAM", _tri, None,
                    "weight gradients on a second stream; None = only in bf16 mode (DESIGN finding 7)"),
    "side_join_first": ("E2_SIDE_JOIN_FIRST", _b, False,
                        "side stream on: the fused first layer's backward waits for the weight gradients on the "
                        "side stream (it runs 62 instead of 35 us beside them, VERDICT r4 weak 9) -- measured: "
                        "bf16 lite183 0.813 -> 0.821 ms, neuro3d 1.144 -> 1.149, unet132 equal: the overlap is "
                        "worth more than the slowdown; off"),
    "side_defer": ("E2_SIDE_DEFER", _b, True,
                   "side stream on: a weight gradient's launches are ISSUED behind the main stream's next "
                   "launches (same dependencies): in the captured graph the main chain then stays on one "
                   "hardware queue (DESIGN finding 54)"),
    "side_mask": ("E2_SIDE_MASK", int, 0,
                  "side stream OFF (f32 mode): bit r set = the weight gradient of the r-th conv layer (forward "
                  "order, fused first layer and head not counted) runs on the side stream all the same"),
    "side_table": ("E2_SIDE_TABLE", _b, True,
                   "side stream OFF (f32 mode): weight gradients whose problem carries a 'side|...' entry in the "
                   "tuning table run on the side stream (tools/tune_side.py measured them inside the step: "
                   "neuro3d_lite's three 200-channel layers, -1.3 % of its step; DESIGN finding 56)"),
    "debug_poison": ("E2_DEBUG_POISON", _b, False,
                     "debugging: the plan's uninitialised buffers (Plan.empty / empty_flat) start as NaN, so "
                     "that a launch reading one before its first writer shows up in the results"),
    "wb_on_side": ("E2_WB_ON_SIDE", _b, True,
                   "bf16 mode: the per-step pack of the bf16 filter rows runs on the side stream beside the "
                   "fused first layer (with the f32 image repack) instead of behind it (finding 54)"),
    "side_pack": ("E2_SIDE_PACK", _b, False, "weight repack as a parallel branch (measured slower)"),
    "fuse_actbwd": ("E2_FUSE_ACTBWD", int, 0, "relu backward in the consumer's dgrad epilogue (finding 17)"),
    "fuse_tail": ("E2_FUSE_TAIL", _b, True, "last 1x1x1 conv + head + loss in one launch (finding 33)"),
    "fuse_multihead": ("E2_FUSE_MULTIHEAD", _b, True,
                       "several MultinoulliNLL terms under one AggregateLoss whose softmaxes sit on (1,1,1) "
                       "'lin' convs of one trunk: all heads, their softmaxes, losses and gradients in one "
                       "launch pair (csrc/multihead.hip); off: the heads run as ordinary conv launches and the "
                       "generic pair of csrc/softmax_nll.hip reads their logits"),
    "bf16_tail": ("E2_BF16_TAIL", _b, True,
                  "bf16 mode: the tail launch too (its two GEMMs round their operands in registers)"),
    "tail_gm": ("E2_TAIL_GM", _b, True, "the tail launch carries its parent's activation backward"),
    "upconv_packed": ("E2_UPCONV_PACKED", _b, True, "UpConv weight images packed by the plan's one repack launch"),
    "concat_alias": ("E2_CONCAT_ALIAS", _b, True, "a concat hands channel slices to parents only it consumes"),
    "pad_inplace": ("E2_PAD_INPLACE", _b, True,
                    "a 'same' / 'full' conv finds its parent's output inside its zero-framed input image "
                    "wherever the parent's producing launch writes a strided view (no pad launch); off: "
                    "every such conv pads by one e2_pad5 launch per step"),
    "zero_in_update": ("E2_ZERO_IN_UPDATE", _b, True, "the optimiser launch clears the gradient arena (finding 38)"),
    "image_stride": ("E2_IMAGE_STRIDE", _b, True,
                     "once a conv launch's tiling is known its packed weight image gets rows as long as that "
                     "tiling's tiles reach (+ 16), not the any-tiling formula (e2_set_image_rows; finding 52)"),
    "pack_rows": ("E2_PACK_ROWS", _b, False,
                  "the repack rewrites the padding rows the TUNED tiling of each launch fetches, not the "
                  "worst case over all tilings (e2_pack_job_set_rows): the repack itself 31 -> 24 us on "
                  "neuro3d, in the step -7 us (neuro3d), -13 us (unet3d_lite), +6 us (neuro3d_lite), "
                  "+-0 (unet3d) -- below the gate; off (DESIGN finding 51)"),
    "adam_pack": ("E2_ADAM_PACK", _b, False,
                  "the Adam launch writes the packed weight images (e2_adam_pack_step); measured slower "
                  "than the two launches it replaces (DESIGN finding 46): off"),
    "dp_overlap": ("E2_DP_OVERLAP", _b, True, "exchange the late layers' gradients under the early backward"),
    "dp_fused_scale": ("E2_DP_FUSED_SCALE", _b, True, "collectives only sum, the optimiser kernel normalises"),
    "bf16_ahead": ("E2_BF16_AHEAD", _b, True, "bf16 mode: producers write the GEMM operands (finding 43)"),
    "bf16_ahead_min": ("E2_BF16_AHEAD_MIN", float, 0.0,
                       "... only when this share of the GEMM launches are memory forms (round 4: 0.6, neuro3d's "
                       "11 of 25 stayed out; with the side stream on a queue of its own -- finding 54 -- engaging "
                       "them pays there too: neuro3d 0.948 -> 0.930 ms, unet3d 6.12 -> 5.84, neuro3d_lite 0.682 -> "
                       "0.640; unet3d_lite 2.44 -> 2.47 is the one that loses)"),
    "bf16_ahead_wgrad_only": ("E2_BF16_AHEAD_WGRAD_ONLY", _b, False, "... gradient images for the weight gradient alone"),
    "bf16_xkeep": ("E2_BF16_XKEEP", _b, True, "bf16 mode: the forward's channels-last copy of x serves the wgrad"),
    "bf16_wpack": ("E2_BF16_WPACK", str, "step", "'step': one filter-row pack launch per step; 'call': per launch"),
    "dense_act_gib": ("E2_DENSE_ACT_GIB", float, 48.0, "activation budget of tiled dense prediction (GiB)"),
}

_set = {}          # process-wide overrides (set_plan_options)


def get(name):
    if name in _set:
        return _set[name]
    env, parse, default, _ = SPEC[name]
    v = os.environ.get(env)
    return default if v is None else parse(v)


def snapshot(overrides=None):
    """all options as a dict (what a Plan keeps)"""
    d = {k: get(k) for k in SPEC}
    for k, v in (overrides or {}).items():
        if k not in SPEC:
            raise KeyError("unknown plan option %r (known: %s)" % (k, ", ".join(sorted(SPEC))))
        d[k] = v
    return d


def set_plan_options(**kw):
    """process-wide defaults of plans constructed from now on; ``name=None`` returns an option
    to its environment / built-in default (except side_stream, where None IS a value: pass
    ``reset=('side_stream',)``)"""
    reset = kw.pop("reset", ())
    for k in reset:
        _set.pop(k, None)
    for k, v in kw.items():
        if k not in SPEC:
            raise KeyError("unknown plan option %r (known: %s)" % (k, ", ".join(sorted(SPEC))))
        if v is None and k != "side_stream":
            _set.pop(k, None)
        else:
            _set[k] = v


@contextlib.contextmanager
def plan_options(**kw):
    """``with plan_options(bf16_ahead=False): ...`` -- plans CONSTRUCTED inside see the values"""
    old = dict(_set)
    try:
        set_plan_options(**kw)
        yield
    finally:
        _set.clear()
        _set.update(old)
