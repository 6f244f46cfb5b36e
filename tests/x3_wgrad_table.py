"""The cases of tests/test_x3_wgrad_instances_gpu.py and tests/test_x3_wgrad_instances_host.py: one literal row per weight-gradient call of the x3 kernels that must land
on one named instance of fx_wgrad_kernel<AIMG, BIMG, MASKED, TAPS, ROWS> or on one of the three kernels for any map width (csrc/p3d_fx.hip) and on one finishing pass of
wgrad_finish (csrc/p3d_conv.hip).  A row is the descriptor, the operands' options, the p3d_fx_tune settings in force during the call and the record
p3d_fx_wgrad_launch_log must hold afterwards, written out as numbers: a change to fx_wgrad_plan / fx_wgrad_two_taps / fx_wgrad_splits / fx_wgrad_order / wgrad_finish
that moves a case off its kernel, its slabs or its finishing pass fails that case by name.  No GPU and no library needed to import this.

Row: name, entry, n, c, k, h, w, r (= s), stride, pad, dil, opts, tune, rec.
entry: 'hook' (the test hook p3d_fx_conv_wgrad_fused), 'stem' / 'stem_masked' (p3d_stem_image(_masked) + p3d_stem_wgrad(_masked): c is Cin, the filter 7x7 stride 2 pad 3).
Options:
  'dyimg' / 'ximg'  the operand as a three-plane image (p3d_fx_act_image, mode 0); with 'rows' as a row image (p3d_fx_row_image); with 'rag' from p3d_fx_act_image_any
  'rag'             the kernels for any map width
  'pm' / 'em'       a per-pixel factor on dy / on x (a partial convolution's mult and mask); an image operand carries its factor: it is built from the fp32 product
  'acc'             accumulate onto a random prior
  'win'             dw is the window c_offset 16 of c_total C + 48 input channels of a wider weight
  'dwoff'           dw is a view one float into a larger buffer: on a 4-byte, not a 16-byte line
tune: ((what, value), ...) of p3d_fx_tune -- (0, n) forces n slabs (cut to the K steps there are, then evened out: ceil(steps / ceil(steps / n))).
Rec: the first 18 fields of one p3d_fx_wgrad_launch_log record (ops.FX_WGRAD_LAUNCH_FIELDS): the plan as p3d_fx_wgrad_plan reports it, the finishing bits, accumulate."""
import collections

Rec = collections.namedtuple('Rec', 'family aimg bimg masked taps rows tile_taps splits spb grid_x grid_y grid_z order tapm slab_bytes_lo slab_bytes_hi finish accumulate')
Row = collections.namedtuple('Row', 'name entry n c k h w r stride pad dil opts tune rec')

ALIGNED, ANY, ANY_MASKED, ANY_IMG = 0, 1, 2, 3                                                # Rec.family
# Rec.finish: the FIN_ bits of wgrad_finish (csrc/p3d_conv.hip), and the stem's own pass
REDUCE, REDUCE_TAPM, REDUCE16, REDUCE16_TAPM, SLAB_FOLD, STEM_DW = 8, 16, 32, 64, 128, 256
FINISH_NAMES = {REDUCE: 'wgrad_reduce', REDUCE_TAPM: 'wgrad_reduce_tapm', REDUCE16: 'wgrad_reduce16', REDUCE16_TAPM: 'wgrad_reduce16_tapm',
                SLAB_FOLD | REDUCE: 'slab_fold + wgrad_reduce', SLAB_FOLD | REDUCE_TAPM: 'slab_fold + wgrad_reduce_tapm', STEM_DW: 'fx_stem_dw'}
OPTIONS = ('dyimg', 'ximg', 'rows', 'rag', 'pm', 'em', 'acc', 'win', 'dwoff')
# the operand bits of p3d_fx_wgrad_plan (include/p3d_hip.h); bit 6: the stem, bit 3 beside it: the masked stem
OPERAND_BITS = dict(dyimg=1, ximg=2, rows=4, pm=8, em=16, rag=32)
STEM_BIT = 64
WINDOW_OFFSET, WINDOW_EXTRA = 16, 48
MAX_TERMS = 3200                # the longest reduction (N * Ho * Wo pixels) X3_TOL (tests/test_kernels_gpu.py) was stated for

# Instances that no row can reach, as (instance tuple, the rule that bars it).  Empty: every compiled weight-gradient kernel is reached by a row below
# (tests/test_x3_wgrad_instances_host.py asserts that this list is exactly the complement of what the rows name).
UNREACHABLE = ()


def instance(rec):
    """the (family, AIMG, BIMG, MASKED, TAPS, ROWS) tuple of a record"""
    return tuple(rec[:6])


def instance_name(inst):
    family, aimg, bimg, masked, taps, rows = inst
    if family != ALIGNED:
        return {ANY: 'fx_wgrad_any_kernel', ANY_MASKED: 'fx_wgrad_any_masked_kernel', ANY_IMG: 'fx_wgrad_any_img_kernel'}.get(family, 'family %d' % family)
    return 'fx_wgrad_kernel<%d, %d, %d, %d, %d>' % (aimg, bimg, masked, taps, rows)


def operand_bits(row):
    if row.entry != 'hook':
        return STEM_BIT | (OPERAND_BITS['pm'] if row.entry == 'stem_masked' else 0)
    return sum(bit for name, bit in OPERAND_BITS.items() if name in row.opts)


ROWS = [
    # fp32 / fp32
    Row('f32_1x1_k200_c144', 'hook', 3, 144, 200, 12, 12, 1, 1, 0, 1, (), (), Rec(0, 0, 0, 0, 0, 0, 0, 1, 27, 2, 2, 1, 0, 0, 115200, 0, 8, 0)),
    Row('f32_3x3_c64_k32_acc', 'hook', 2, 64, 32, 8, 12, 3, 1, 1, 1, ('acc',), (), Rec(0, 0, 0, 0, 0, 0, 0, 1, 12, 1, 1, 9, 0, 1, 73728, 0, 16, 1)),
    Row('f32_3x3_stride2', 'hook', 3, 64, 96, 12, 16, 3, 2, 1, 1, (), (), Rec(0, 0, 0, 0, 0, 0, 0, 1, 9, 1, 1, 9, 0, 1, 221184, 0, 16, 0)),
    Row('f32_1x1_stride2', 'hook', 3, 32, 144, 12, 16, 1, 2, 0, 1, (), (), Rec(0, 0, 0, 0, 0, 0, 0, 1, 9, 1, 2, 1, 0, 0, 18432, 0, 8, 0)),
    Row('f32_dil2', 'hook', 1, 64, 128, 12, 8, 3, 1, 2, 2, (), (), Rec(0, 0, 0, 0, 0, 0, 0, 1, 6, 1, 1, 9, 0, 1, 294912, 0, 16, 0)),
    Row('f32_5x5', 'hook', 2, 64, 48, 8, 8, 5, 1, 2, 1, (), (), Rec(0, 0, 0, 0, 0, 0, 0, 1, 8, 1, 1, 25, 0, 1, 307200, 0, 16, 0)),
    Row('f32_split4_uneven', 'hook', 3, 144, 200, 12, 12, 1, 1, 0, 1, (), ((0, 4),), Rec(0, 0, 0, 0, 0, 0, 0, 4, 7, 2, 2, 4, 0, 0, 460800, 0, 8, 0)),
    Row('f32_1x1_slabs18', 'hook', 18, 32, 80, 4, 4, 1, 1, 0, 1, (), ((0, 18),), Rec(0, 0, 0, 0, 0, 0, 0, 18, 1, 1, 1, 18, 0, 0, 184320, 0, 32, 0)),
    Row('f32_1x1_slabs18_window_acc', 'hook', 18, 32, 80, 4, 4, 1, 1, 0, 1, ('win', 'acc'), ((0, 18),), Rec(0, 0, 0, 0, 0, 0, 0, 18, 1, 1, 1, 18, 0, 0, 184320, 0, 136, 1)),
    Row('f32_1x1_slabs18_dwoff', 'hook', 18, 32, 80, 4, 4, 1, 1, 0, 1, ('dwoff',), ((0, 18),), Rec(0, 0, 0, 0, 0, 0, 0, 18, 1, 1, 1, 18, 0, 0, 184320, 0, 136, 0)),
    Row('f32_1x1_window_unsplit', 'hook', 2, 32, 96, 8, 8, 1, 1, 0, 1, ('win',), (), Rec(0, 0, 0, 0, 0, 0, 0, 1, 8, 1, 1, 1, 0, 0, 12288, 0, 8, 0)),
    Row('f32_3x3_slabs17_uneven_acc', 'hook', 11, 64, 32, 4, 12, 3, 1, 1, 1, ('acc',), ((0, 17),), Rec(0, 0, 0, 0, 0, 0, 0, 17, 2, 1, 1, 153, 0, 1, 1253376, 0, 64, 1)),
    Row('f32_9x9_slabs18', 'hook', 18, 64, 32, 4, 4, 9, 1, 4, 1, (), ((0, 18),), Rec(0, 0, 0, 0, 0, 0, 0, 18, 1, 1, 1, 1458, 0, 1, 11943936, 0, 144, 0)),
    Row('f32_order1_c512_k200', 'hook', 2, 512, 200, 4, 4, 3, 1, 1, 1, (), (), Rec(0, 0, 0, 0, 0, 0, 0, 1, 2, 4, 2, 9, 1, 1, 3686400, 0, 16, 0)),
    Row('f32_order1_split2', 'hook', 2, 512, 200, 4, 4, 3, 1, 1, 1, (), ((0, 2),), Rec(0, 0, 0, 0, 0, 0, 0, 2, 1, 4, 2, 18, 1, 1, 7372800, 0, 16, 0)),
    # masked fp32
    Row('f32_masked_3x3', 'hook', 3, 64, 64, 12, 12, 3, 1, 1, 1, ('pm', 'em'), (), Rec(0, 0, 0, 1, 0, 0, 0, 1, 27, 1, 1, 9, 0, 1, 147456, 0, 16, 0)),
    Row('f32_masked_1x1_stride2_split2', 'hook', 4, 32, 96, 8, 16, 1, 2, 0, 1, ('pm', 'em'), ((0, 2),), Rec(0, 0, 0, 1, 0, 0, 0, 2, 4, 1, 1, 2, 0, 0, 24576, 0, 8, 0)),
    Row('f32_masked_dil2_acc', 'hook', 2, 64, 48, 12, 8, 3, 1, 2, 2, ('pm', 'em', 'acc'), (), Rec(0, 0, 0, 1, 0, 0, 0, 1, 12, 1, 1, 9, 0, 1, 110592, 0, 16, 1)),
    # dy image, fp32 x
    Row('dyimg_1x1_k80_c36', 'hook', 3, 36, 80, 12, 12, 1, 1, 0, 1, ('dyimg',), (), Rec(0, 1, 0, 0, 0, 0, 0, 1, 27, 1, 1, 1, 0, 0, 11520, 0, 8, 0)),
    Row('dyimg_3x3_stride2', 'hook', 3, 64, 96, 12, 16, 3, 2, 1, 1, ('dyimg',), (), Rec(0, 1, 0, 0, 0, 0, 0, 1, 9, 1, 1, 9, 0, 1, 221184, 0, 16, 0)),
    Row('dyrows_1x1', 'hook', 3, 48, 80, 12, 12, 1, 1, 0, 1, ('dyimg', 'rows'), (), Rec(0, 1, 0, 0, 0, 1, 0, 1, 27, 1, 1, 1, 0, 0, 15360, 0, 8, 0)),
    Row('dyrows_3x3_split3_acc', 'hook', 5, 64, 48, 8, 8, 3, 1, 1, 1, ('dyimg', 'rows', 'acc'), ((0, 3),), Rec(0, 1, 0, 0, 0, 1, 0, 3, 7, 1, 1, 27, 0, 1, 331776, 0, 16, 1)),
    Row('dyimg_xmask_3x3', 'hook', 3, 64, 64, 12, 12, 3, 1, 1, 1, ('dyimg', 'em'), (), Rec(0, 1, 0, 1, 0, 0, 0, 1, 27, 1, 1, 9, 0, 1, 147456, 0, 16, 0)),
    Row('dyimg_xmask_1x1_c40_split3_acc', 'hook', 3, 40, 80, 12, 12, 1, 1, 0, 1, ('dyimg', 'em', 'acc'), ((0, 3),), Rec(0, 1, 0, 1, 0, 0, 0, 3, 9, 1, 1, 3, 0, 0, 38400, 0, 8, 1)),
    # both images, one tap per block
    Row('img_1x1_k208_c144', 'hook', 3, 144, 208, 12, 12, 1, 1, 0, 1, ('dyimg', 'ximg'), (), Rec(0, 1, 1, 0, 0, 0, 0, 1, 27, 2, 2, 1, 0, 0, 119808, 0, 8, 0)),
    Row('img_3x3_c128_k80_stride2', 'hook', 3, 128, 80, 12, 16, 3, 2, 1, 1, ('dyimg', 'ximg'), (), Rec(0, 1, 1, 0, 0, 0, 0, 1, 9, 1, 1, 9, 0, 1, 368640, 0, 16, 0)),
    Row('img_3x3_c64_w12', 'hook', 2, 64, 64, 8, 12, 3, 1, 1, 1, ('dyimg', 'ximg'), (), Rec(0, 1, 1, 0, 0, 0, 0, 1, 12, 1, 1, 9, 0, 1, 147456, 0, 16, 0)),
    Row('rows_1x1_k80_c48', 'hook', 3, 48, 80, 12, 12, 1, 1, 0, 1, ('dyimg', 'ximg', 'rows'), (), Rec(0, 1, 1, 0, 0, 1, 0, 1, 27, 1, 1, 1, 0, 0, 15360, 0, 8, 0)),
    Row('rows_3x3_c128_dil2_acc', 'hook', 2, 128, 48, 12, 8, 3, 1, 2, 2, ('dyimg', 'ximg', 'rows', 'acc'), (), Rec(0, 1, 1, 0, 0, 1, 0, 1, 12, 1, 1, 9, 0, 1, 221184, 0, 16, 1)),
    Row('img_order1_c512', 'hook', 2, 512, 48, 4, 4, 3, 1, 1, 1, ('dyimg', 'ximg'), (), Rec(0, 1, 1, 0, 0, 0, 0, 1, 2, 4, 1, 9, 1, 1, 884736, 0, 16, 0)),
    Row('img_1x1_slabs18', 'hook', 18, 32, 80, 4, 4, 1, 1, 0, 1, ('dyimg', 'ximg'), ((0, 18),), Rec(0, 1, 1, 0, 0, 0, 0, 18, 1, 1, 1, 18, 0, 0, 184320, 0, 32, 0)),
    # TAPS 3: C = 64, K <= 64, Wo % 16 == 0
    Row('t3_3x3_k64', 'hook', 2, 64, 64, 4, 16, 3, 1, 1, 1, ('dyimg', 'ximg'), (), Rec(0, 1, 1, 0, 3, 0, 3, 1, 8, 3, 1, 1, 0, 1, 147456, 0, 16, 0)),
    Row('t3_3x3_k48_acc', 'hook', 2, 64, 48, 4, 16, 3, 1, 1, 1, ('dyimg', 'ximg', 'acc'), (), Rec(0, 1, 1, 0, 3, 0, 3, 1, 8, 3, 1, 1, 0, 1, 110592, 0, 16, 1)),
    Row('t3_5x5_k32', 'hook', 1, 64, 32, 4, 16, 5, 1, 2, 1, ('dyimg', 'ximg'), (), Rec(0, 1, 1, 0, 3, 0, 3, 1, 4, 9, 1, 1, 0, 1, 204800, 0, 16, 0)),
    Row('t3_rows_3x3_stride2', 'hook', 2, 64, 64, 8, 32, 3, 2, 1, 1, ('dyimg', 'ximg', 'rows'), (), Rec(0, 1, 1, 0, 3, 1, 3, 1, 8, 3, 1, 1, 0, 1, 147456, 0, 16, 0)),
    Row('t3_split3_uneven', 'hook', 5, 64, 64, 4, 16, 3, 1, 1, 1, ('dyimg', 'ximg'), ((0, 3),), Rec(0, 1, 1, 0, 3, 0, 3, 3, 7, 3, 1, 3, 0, 1, 442368, 0, 16, 0)),
    # TAPS 2: C = 64, K > 64
    Row('t2_3x3_k80', 'hook', 2, 64, 80, 4, 16, 3, 1, 1, 1, ('dyimg', 'ximg'), (), Rec(0, 1, 1, 0, 2, 0, 2, 1, 8, 5, 1, 1, 0, 1, 184320, 0, 16, 0)),
    Row('t2_3x3_k208', 'hook', 2, 64, 208, 4, 16, 3, 1, 1, 1, ('dyimg', 'ximg'), (), Rec(0, 1, 1, 0, 2, 0, 2, 1, 8, 5, 2, 1, 0, 1, 479232, 0, 16, 0)),
    Row('t2_rows_5x5_k96', 'hook', 1, 64, 96, 4, 16, 5, 1, 2, 1, ('dyimg', 'ximg', 'rows'), (), Rec(0, 1, 1, 0, 2, 1, 2, 1, 4, 13, 1, 1, 0, 1, 614400, 0, 16, 0)),
    Row('t2_slabs18_acc', 'hook', 9, 64, 80, 4, 16, 3, 1, 1, 1, ('dyimg', 'ximg', 'acc'), ((0, 18),), Rec(0, 1, 1, 0, 2, 0, 2, 18, 2, 5, 1, 18, 0, 1, 3317760, 0, 64, 1)),
    # any map width
    Row('any_1x1_5x7', 'hook', 3, 100, 99, 5, 7, 1, 1, 0, 1, ('rag',), (), Rec(1, 0, 0, 0, 0, 0, 0, 1, 7, 1, 1, 1, 0, 0, 39600, 0, 8, 0)),
    Row('any_3x3_9x9_acc', 'hook', 2, 64, 100, 9, 9, 3, 1, 1, 1, ('rag', 'acc'), (), Rec(1, 0, 0, 0, 0, 0, 0, 1, 11, 1, 1, 9, 0, 1, 230400, 0, 16, 1)),
    Row('any_3x3_stride2_9x9', 'hook', 2, 64, 48, 9, 9, 3, 2, 1, 1, ('rag',), (), Rec(1, 0, 0, 0, 0, 0, 0, 1, 4, 1, 1, 9, 0, 1, 110592, 0, 16, 0)),
    Row('any_split3_uneven', 'hook', 3, 100, 99, 5, 7, 1, 1, 0, 1, ('rag',), ((0, 3),), Rec(1, 0, 0, 0, 0, 0, 0, 3, 3, 1, 1, 3, 0, 0, 118800, 0, 8, 0)),
    Row('any_one_partial_step', 'hook', 1, 32, 32, 3, 5, 1, 1, 0, 1, ('rag',), (), Rec(1, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 0, 0, 4096, 0, 8, 0)),
    Row('any_masked_3x3_9x9', 'hook', 2, 64, 64, 9, 9, 3, 1, 1, 1, ('rag', 'pm', 'em'), (), Rec(2, 0, 0, 0, 0, 0, 0, 1, 11, 1, 1, 9, 0, 1, 147456, 0, 16, 0)),
    Row('any_masked_1x1_5x7_acc_split2', 'hook', 3, 40, 80, 5, 7, 1, 1, 0, 1, ('rag', 'pm', 'em', 'acc'), ((0, 2),), Rec(2, 0, 0, 0, 0, 0, 0, 2, 4, 1, 1, 2, 0, 0, 25600, 0, 8, 1)),
    Row('anyimg_1x1_5x7_k112_c48', 'hook', 3, 48, 112, 5, 7, 1, 1, 0, 1, ('rag', 'dyimg', 'ximg'), (), Rec(3, 0, 0, 0, 0, 0, 0, 1, 7, 1, 1, 1, 0, 0, 21504, 0, 8, 0)),
    Row('anyimg_3x3_9x9_acc', 'hook', 2, 64, 96, 9, 9, 3, 1, 1, 1, ('rag', 'dyimg', 'ximg', 'acc'), (), Rec(3, 0, 0, 0, 0, 0, 0, 1, 11, 1, 1, 9, 0, 1, 221184, 0, 16, 1)),
    Row('anyimg_split2', 'hook', 2, 64, 96, 9, 9, 3, 1, 1, 1, ('rag', 'dyimg', 'ximg'), ((0, 2),), Rec(3, 0, 0, 0, 0, 0, 0, 2, 6, 1, 1, 18, 0, 1, 442368, 0, 16, 0)),
    Row('anyimg_aligned_8x8', 'hook', 2, 64, 96, 8, 8, 3, 1, 1, 1, ('rag', 'dyimg', 'ximg'), (), Rec(3, 0, 0, 0, 0, 0, 0, 1, 8, 1, 1, 9, 0, 1, 221184, 0, 16, 0)),
    # the stem
    Row('stem_rgb_k64', 'stem', 2, 3, 64, 8, 16, 7, 2, 3, 1, (), (), Rec(0, 0, 1, 0, 1, 0, 8, 1, 4, 2, 1, 1, 0, 1, 65536, 0, 256, 0)),
    Row('stem_depth_k80_acc', 'stem', 2, 1, 80, 8, 16, 7, 2, 3, 1, ('acc',), (), Rec(0, 0, 1, 0, 1, 0, 8, 1, 4, 2, 1, 1, 0, 1, 81920, 0, 256, 1)),
    Row('stem_masked_k32_two_slabs', 'stem_masked', 4, 3, 32, 32, 32, 7, 2, 3, 1, (), (), Rec(0, 0, 1, 1, 1, 0, 8, 2, 32, 2, 1, 2, 0, 1, 65536, 0, 256, 0)),
]
