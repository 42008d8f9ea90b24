"""How an all-pairs pass chooses its kernel and its strip form, written down a second time: the oracle of
tests/test_pass_form.py (against choose_pass and the StripForm table of storm_hip_plan.*, without a device) and of
tests/test_gpu_pass_form.py (against what the library reports after a call). Nothing here is generated from the C++.

Kernel families: "popcount", "fp4_tiles", "fp4_strips" (256-row A tiles), "fp4_strips_wide" (512), "k2q", "k2b" (with a
form: "bits", "bits_wide" or "rows"), and the two forms of the tools build, "tools_stripbits" (k2_strip_operands 1) and
"tools_bitwave" (3)."""
from collections import namedtuple

# ---- the strip forms: one row each ----------------------------------------------------------------------------------------
# slices: k-slices that hold data for rows of w words; slice_words: the pass report's words per slice; wave_sum_max: the most
# a wave adds to a slot; operands / rows: what k2_operands_used / k2_strip_rows_used say after a launch; plan: the form number
# of dist.strip_plan. None: the form has no such number.
Form = namedtuple("Form", "kernel a_tile waves threads slices slice_words xcd_group wave_sum_max operands rows plan")
FORMS = {
    "fp4": Form("strip16_fp4_kernel", 256, 4, 256, lambda w: (w + 3) // 4, None, 1, None, 4, None, 0),
    "bits": Form("strip16_bits_kernel", 256, 4, 256, lambda w: 2 * ((w + 7) // 8), 4, 2, 64 * (4096 * 64 + 256) * 256, 5, 64, 1),
    "bits_wide": Form("strip16_bits2_kernel", 512, 8, 512, lambda w: 2 * ((w + 7) // 8), 4, 2, 64 * (4096 * 64 + 256) * 256, 6, 64,
                      None),
    "rows": Form("strip16_rows_kernel", 512, 4, 256, lambda w: (w + 1) // 2, 2, 8, 128 * (4096 * 64 + 512) * 128, 5, 128, 2),
}

# what storm_hip_last_pass_report names for a family (every K2b form reports as the bit strips)
REPORTED = {"popcount": "pairw_dense_kernel", "fp4_tiles": "pairw_fp4_kernel", "fp4_strips": "strip16_fp4_kernel",
            "fp4_strips_wide": "strip16_fp4_kernel", "k2q": "bitstream_kernel", "k2b": "strip16_bits_kernel"}

Options = namedtuple("Options", "variant k2_strip_operands k2_strip_rows k2_ring k2_shape k2_persistent k2_debug tools")
Options.__new__.__defaults__ = (-1, 0, 0, 4, 16, 0, 0, False)
# dense and dense-upload: the matrix; the sparse pool: rows_dst, pool_rows_ready and the widest block column
Shape = namedtuple("Shape", "n_rows n_rows_pad n_words stride_words shard_count rows_dst pool_rows_ready widest")
Shape.__new__.__defaults__ = (0, 256, 1, 64, 1, 0, 0, 0)
# operands_used None: the pass leaves k2_operands_used as it was; in_panels: dense-upload only
Choice = namedtuple("Choice", "family form variant_used operands_used in_panels")


def allocation(n_rows):
    """rows a fresh matrix of n_rows allocates: a multiple of 256, at least 256"""
    return max(256, (n_rows + 255) // 256 * 256)


def stride(n_words):
    """allocated words per row: a multiple of 64"""
    return (n_words + 63) // 64 * 64


def _pad(s, t):
    return (s.n_rows + t - 1) // t * t <= s.n_rows_pad


def _ops(o):
    """(ops, wide asked for)"""
    if o.k2_strip_operands == 6:
        return 5, True
    if o.k2_strip_operands == 0:
        return (5 if (o.k2_ring, o.k2_shape) == (4, 16) else 4), False
    return o.k2_strip_operands, False


def _bit_operands(o, s):
    return not o.k2_persistent and o.k2_debug == 0 and _pad(s, 256) and s.stride_words * 8 * 64 < 2 ** 32


def _dense(o, s):
    variant = 4 if o.variant == -1 else o.variant
    if variant <= 2:
        return Choice("popcount", None, variant, None, False)
    if variant == 3:
        return Choice("fp4_tiles", None, 3, 4, False)
    if variant == 5:
        return Choice("fp4_strips_wide", None, 5, 4, False)
    ops, wide = _ops(o)
    if ops not in (1, 2, 3, 5) or not _bit_operands(o, s):
        return Choice("fp4_strips", None, 4, 4, False)
    if ops == 2:
        return Choice("k2q", None, 4, 2, False)
    if ops == 1 or (ops == 3 and not o.tools):    # the shipped library refuses both with the text of 1
        return Choice("tools_stripbits", None, 4, ops, False)
    if ops == 3:
        return Choice("tools_bitwave", None, 4, 3, False)
    if wide:
        form = "bits_wide" if _pad(s, 512) else "bits"
    elif o.k2_strip_rows != 64 and _pad(s, 512) and \
            (o.k2_strip_rows == 128 or (s.shard_count == 1 and s.n_rows >= 2048 and s.n_words >= 1024)):
        form = "rows"
    else:
        form = "bits"
    return Choice("k2b", form, 4, FORMS[form].operands, False)


def choose(caller, o, s):
    """caller: "dense", "upload" or "pool"."""
    if caller == "dense":
        return _dense(o, s)
    if caller == "upload":
        if o.variant in (-1, 4) and _ops(o)[0] == 5 and not o.k2_persistent and o.k2_debug == 0 and s.n_rows >= 2048 and \
                _pad(s, 256) and s.stride_words * 8 * 64 < 2 ** 32:
            return Choice("k2b", "bits", 4, 5, True)
        return _dense(o, s)    # the copy, then the dense pass
    assert caller == "pool"
    variant = o.variant if o.variant != -1 else (4 if s.widest >= 64 else 2)
    if variant <= 2:
        return Choice("popcount", None, variant, None, False)
    if variant == 4 and _ops(o)[0] == 5 and o.k2_debug == 0 and not o.k2_persistent and s.rows_dst <= s.pool_rows_ready + 512:
        return Choice("k2b", "bits", 4, 5, False)
    return Choice({3: "fp4_tiles", 4: "fp4_strips", 5: "fp4_strips_wide"}[variant], None, variant, None, False)
