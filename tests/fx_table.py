"""The cases of tests/test_fx_instances_gpu.py and tests/test_fx_instances_host.py: one literal row per call of p3d_fx_conv_fused (the test hook that reaches fx_conv_fwd /
fx_conv_dgrad of csrc/p3d_fx.hip with any fusion) that must land on one named instance of fx_conv_kernel / fx16_conv_kernel and its finishing pass.  A row is the
descriptor, the operands' options, the p3d_fx_tune settings in force during the call and the records p3d_fx_launch_log must hold afterwards, written out as numbers: a
change to fx_plan / fx16_bm / fx_select / FX_TAP_INNER_MIN that moves a case off its instance fails that case by name.  No GPU and no library needed to import this.

Row: name, pass_ ('fwd' / 'dgrad'), n, c, k, h, w, r (= s), stride, pad, dil, opts, tune, recs.
Options:
  operand   'img' (three-plane activation image), 'rows' (fp32 row image); neither: the fp32 tensor.  'rag': the ragged instances (any map width)
  weights   'wimg' (a cached weight image; otherwise built into the workspace), 'win' (the C channels are the window c_offset 16 of c_total C + 48 of the weight)
  epilogue  'bias'; 'acc' (accumulate onto what the result held); 'accsrc' (data gradient: accumulate from another tensor), with 'accmask' through mask bytes;
            'factor' (partial convolution: result factor, and the operand factor for an fp32 operand; some windows wholly empty, factor 0); 'sums' (the partial
            sums of the BatchNorm epilogues); 'infer' with 'res' / 'relu' (the inference tail)
  'long'    a reduction longer than the 3200 terms X3_TOL was stated for (>= 1024 channels x 9 taps: the tap-inner order): judged against the fp32-MFMA kernel's error
tune: ((what, value), ...) of p3d_fx_tune -- (1, n) forces n split-K slabs (1: unsplit), (5, 1) one launch per parity class of a strided data gradient.
Rec: the fields of one p3d_fx_launch_log record (ops.FX_LAUNCH_FIELDS)."""
import collections

Rec = collections.namedtuple('Rec', 'kernel amode pro epi tapi rag rows grid_x grid_y grid_z kchunk finish finish_groups')       # ops.FX_LAUNCH_FIELDS
Row = collections.namedtuple('Row', 'name pass_ n c k h w r stride pad dil opts tune recs')

# epilogue codes (csrc/p3d_fx.h) and what follows a split launch (include/p3d_hip.h)
STORE, STATS, BWD_SUMS, FACTOR, FACTOR_STATS, FACTOR_BWD_SUMS, FACTOR_IMG, INFER, INFER_FACTOR = 0, 1, 2, 4, 5, 6, 7, 8, 9
EPI_NAMES = {STORE: 'STORE', STATS: 'STATS', BWD_SUMS: 'BWD_SUMS', FACTOR: 'FACTOR', FACTOR_STATS: 'FACTOR_STATS', FACTOR_BWD_SUMS: 'FACTOR_BWD_SUMS',
             FACTOR_IMG: 'FACTOR_IMG', INFER: 'INFER', INFER_FACTOR: 'INFER_FACTOR'}
NO_FINISH, REDUCE0, REDUCE1, REDUCE2, REDUCE_ANY = 0, 1, 2, 3, 4
OPTIONS = ('img', 'rows', 'rag', 'wimg', 'win', 'bias', 'acc', 'accsrc', 'accmask', 'factor', 'sums', 'infer', 'res', 'relu', 'long')
WINDOW_OFFSET, WINDOW_EXTRA = 16, 48
MAX_TERMS = 3200                # the longest reduction X3_TOL (tests/test_kernels_gpu.py) was stated for; rows beyond it carry 'long'
TAP_INNER_MIN = 1024            # FX_TAP_INNER_MIN of csrc/p3d_fx.hip

# Instances that fx_conv_fwd / fx_conv_dgrad cannot launch whatever they are given, as (instance tuple, the P3D_REQUIRE or rule that bars it).  Empty: every compiled
# instance is reached by a row below (tests/test_fx_instances_host.py asserts that this list is exactly the complement of what the rows name).
UNREACHABLE = ()


def instance(rec):
    """the (kernel, AMODE, PRO, EPI, TAPI, RAG, ROWS) tuple of a record, as p3d_fx_conv_instances lists them"""
    return tuple(rec[:7])


def instance_name(inst):
    kernel, amode, pro, epi, tapi, rag, rows = inst
    head = 'fx_conv_kernel<%d, %d, ' % (amode, pro) if kernel == 0 else 'fx16_conv_kernel<%d, ' % kernel
    tail = ', %d, %d, %d>' % (tapi, rag, rows) if kernel == 0 else ', %d, %d>' % (tapi, rows)
    return head + EPI_NAMES.get(epi, str(epi)) + tail


ROWS = [
    Row('f32_fwd_store_1x1_bias', 'fwd', 3, 32, 200, 12, 12, 1, 1, 0, 1, ('bias',), (), (Rec(0, 0, 0, STORE, 0, 0, 0, 8, 1, 1, 0, 0, 0),)),
    Row('f32_fwd_store_3x3_window_acc', 'fwd', 2, 32, 96, 8, 12, 3, 1, 1, 1, ('win', 'acc'), (), (Rec(0, 0, 0, STORE, 0, 0, 0, 2, 1, 1, 0, 0, 0),)),
    Row('f32_fwd_store_dil2_bias_acc', 'fwd', 1, 48, 128, 12, 8, 3, 1, 2, 2, ('bias', 'acc'), (), (Rec(0, 0, 0, STORE, 0, 0, 0, 1, 1, 1, 0, 0, 0),)),
    Row('f32_fwd_store_exact_tile', 'fwd', 2, 32, 320, 8, 8, 1, 1, 0, 1, ('wimg',), (), (Rec(0, 0, 0, STORE, 0, 0, 0, 3, 1, 1, 0, 0, 0),)),
    Row('f32_fwd_store_stride2_3x3', 'fwd', 3, 32, 96, 12, 16, 3, 2, 1, 1, ('bias',), (), (Rec(0, 0, 0, STORE, 0, 0, 0, 2, 1, 1, 0, 0, 0),)),
    Row('f32_fwd_store_stride2_1x1', 'fwd', 3, 32, 144, 12, 16, 1, 2, 0, 1, ('wimg',), (), (Rec(0, 0, 0, STORE, 0, 0, 0, 4, 1, 1, 0, 0, 0),)),
    Row('f32_fwd_stats_1x1_bias', 'fwd', 3, 32, 200, 12, 12, 1, 1, 0, 1, ('sums', 'bias'), (), (Rec(0, 0, 0, STATS, 0, 0, 0, 8, 1, 1, 0, 0, 0),)),
    Row('f32_fwd_stats_3x3_w4', 'fwd', 7, 32, 100, 6, 4, 3, 1, 1, 1, ('sums', 'wimg'), (), (Rec(0, 0, 0, STATS, 0, 0, 0, 2, 1, 1, 0, 0, 0),)),
    Row('f32_dgrad_store_3x3_acc', 'dgrad', 3, 96, 32, 12, 12, 3, 1, 1, 1, ('acc',), (), (Rec(0, 0, 0, STORE, 0, 0, 0, 4, 1, 1, 0, 0, 0),)),
    Row('f32_dgrad_bwdsums_1x1', 'dgrad', 3, 200, 32, 12, 12, 1, 1, 0, 1, ('sums',), (), (Rec(0, 0, 0, BWD_SUMS, 0, 0, 0, 8, 1, 1, 0, 0, 0),)),
    Row('f32_dgrad_bwdsums_3x3', 'dgrad', 2, 96, 48, 8, 12, 3, 1, 1, 1, ('sums', 'wimg'), (), (Rec(0, 0, 0, BWD_SUMS, 0, 0, 0, 2, 1, 1, 0, 0, 0),)),
    Row('f32_dgrad_accsrc_mask', 'dgrad', 3, 144, 32, 12, 12, 1, 1, 0, 1, ('accsrc', 'accmask'), (), (Rec(0, 0, 0, STORE, 0, 0, 0, 8, 1, 1, 0, 0, 0),)),
    Row('f32_fwd_infer_3x3_bias_res_relu', 'fwd', 3, 32, 200, 12, 12, 3, 1, 1, 1, ('infer', 'wimg', 'bias', 'res', 'relu'), (), (Rec(0, 0, 0, INFER, 0, 0, 0, 8, 1, 1, 0, 0, 0),)),
    Row('f32_fwd_infer_1x1_bias_acc', 'fwd', 2, 48, 80, 8, 12, 1, 1, 0, 1, ('infer', 'wimg', 'bias', 'acc'), (), (Rec(0, 0, 0, INFER, 0, 0, 0, 2, 1, 1, 0, 0, 0),)),
    Row('f32_fwd_factor_3x3', 'fwd', 3, 32, 64, 12, 12, 3, 1, 1, 1, ('factor',), (), (Rec(0, 0, 4, FACTOR, 0, 0, 0, 4, 1, 1, 0, 0, 0),)),
    Row('f32_fwd_factor_acc', 'fwd', 2, 32, 144, 8, 12, 3, 1, 1, 1, ('factor', 'acc'), (), (Rec(0, 0, 4, FACTOR, 0, 0, 0, 4, 1, 1, 0, 0, 0),)),
    Row('f32_dgrad_factor_3x3_acc', 'dgrad', 3, 72, 32, 12, 12, 3, 1, 1, 1, ('factor', 'acc'), (), (Rec(0, 0, 4, FACTOR, 0, 0, 0, 4, 1, 1, 0, 0, 0),)),
    Row('f32_dgrad_factor_dil2', 'dgrad', 2, 64, 48, 12, 8, 3, 1, 2, 2, ('factor', 'wimg'), (), (Rec(0, 0, 4, FACTOR, 0, 0, 0, 2, 1, 1, 0, 0, 0),)),
    Row('f32_fwd_factor_stats', 'fwd', 3, 32, 80, 12, 12, 3, 1, 1, 1, ('factor', 'sums'), (), (Rec(0, 0, 4, FACTOR_STATS, 0, 0, 0, 4, 1, 1, 0, 0, 0),)),
    Row('f32_fwd_infer_factor_bias_res_relu', 'fwd', 3, 32, 64, 12, 12, 3, 1, 1, 1, ('infer', 'wimg', 'factor', 'bias', 'res', 'relu'), (), (Rec(0, 0, 4, INFER_FACTOR, 0, 0, 0, 4, 1, 1, 0, 0, 0),)),
    Row('f32_fwd_infer_factor_bias', 'fwd', 2, 32, 200, 8, 12, 3, 1, 1, 1, ('infer', 'wimg', 'factor', 'bias'), (), (Rec(0, 0, 4, INFER_FACTOR, 0, 0, 0, 4, 1, 1, 0, 0, 0),)),
    Row('f32_fwd_split2_bias', 'fwd', 3, 64, 200, 12, 12, 1, 1, 0, 1, ('bias',), ((1, 2),), (Rec(0, 0, 0, STORE, 0, 0, 0, 8, 2, 1, 2, 1, 3),)),
    Row('f32_fwd_split4_uneven_stats_n18', 'fwd', 18, 32, 80, 4, 4, 3, 1, 1, 1, ('sums', 'bias'), ((1, 4),), (Rec(0, 0, 0, STORE, 0, 0, 0, 3, 4, 1, 5, 2, 16),)),
    Row('f32_dgrad_split2_bwdsums_n18', 'dgrad', 18, 80, 32, 4, 4, 1, 1, 0, 1, ('sums',), ((1, 2),), (Rec(0, 0, 0, STORE, 0, 0, 0, 3, 2, 1, 1, 3, 16),)),
    Row('f32_dgrad_split4_uneven_bwdsums_n3', 'dgrad', 3, 144, 32, 12, 12, 3, 1, 1, 1, ('sums', 'wimg'), ((1, 4),), (Rec(0, 0, 0, STORE, 0, 0, 0, 8, 4, 1, 5, 3, 3),)),
    Row('f32_dgrad_split2_acc', 'dgrad', 3, 96, 64, 12, 12, 1, 1, 0, 1, ('acc',), ((1, 2),), (Rec(0, 0, 0, STORE, 0, 0, 0, 4, 2, 1, 2, 1, 3),)),
    Row('f32_fwd_split2_factor_acc', 'fwd', 3, 32, 64, 12, 12, 3, 1, 1, 1, ('factor', 'acc'), ((1, 2),), (Rec(0, 0, 4, STORE, 0, 0, 0, 4, 2, 1, 9, 1, 3),)),
    Row('f32_fwd_split4_uneven_factor_stats_n18', 'fwd', 18, 32, 80, 4, 4, 3, 1, 1, 1, ('factor', 'sums'), ((1, 4),), (Rec(0, 0, 4, STORE, 0, 0, 0, 3, 4, 1, 5, 2, 16),)),
    Row('f32_dgrad_split2_factor', 'dgrad', 3, 72, 32, 12, 12, 3, 1, 1, 1, ('factor',), ((1, 2),), (Rec(0, 0, 4, STORE, 0, 0, 0, 4, 2, 1, 9, 1, 3),)),
    Row('f32_fwd_split2_infer_bias_res_relu', 'fwd', 3, 64, 200, 12, 12, 1, 1, 0, 1, ('infer', 'wimg', 'bias', 'res', 'relu'), ((1, 2),), (Rec(0, 0, 0, STORE, 0, 0, 0, 8, 2, 1, 2, 1, 3),)),
    Row('f32_fwd_split4_uneven_infer_factor_n18', 'fwd', 18, 32, 64, 4, 4, 3, 1, 1, 1, ('infer', 'wimg', 'factor', 'bias', 'res', 'relu'), ((1, 4),), (Rec(0, 0, 4, STORE, 0, 0, 0, 3, 4, 1, 5, 1, 16),)),
    Row('f32_fwd_split_planned_3x3_c128', 'fwd', 2, 128, 96, 8, 8, 3, 1, 1, 1, ('bias',), (), (Rec(0, 0, 0, STORE, 0, 0, 0, 1, 2, 1, 36, 1, 2),)),
    Row('f32_dgrad_stride2_3x3_classes', 'dgrad', 3, 96, 32, 12, 16, 3, 2, 1, 1, (), (), (Rec(0, 0, 0, STORE, 0, 0, 0, 2, 1, 4, 0, 0, 0),)),
    Row('f32_dgrad_stride2_3x3_acc', 'dgrad', 2, 200, 32, 8, 16, 3, 2, 1, 1, ('acc',), (), (Rec(0, 0, 0, STORE, 0, 0, 0, 2, 1, 4, 0, 0, 0),)),
    Row('f32_dgrad_stride2_3x3_class_launches', 'dgrad', 3, 96, 32, 12, 16, 3, 2, 1, 1, (), ((5, 1),), (Rec(0, 0, 0, STORE, 0, 0, 0, 2, 1, 1, 0, 0, 0), Rec(0, 0, 0, STORE, 0, 0, 0, 2, 1, 1, 0, 0, 0), Rec(0, 0, 0, STORE, 0, 0, 0, 2, 1, 1, 0, 0, 0), Rec(0, 0, 0, STORE, 0, 0, 0, 2, 1, 1, 0, 0, 0),)),
    Row('f32_dgrad_stride2_1x1_dead_classes', 'dgrad', 3, 144, 32, 12, 16, 1, 2, 0, 1, (), (), (Rec(0, 0, 0, STORE, 0, 0, 0, 4, 1, 1, 0, 0, 0),)),
    Row('f32_dgrad_stride2_1x1_class_launches', 'dgrad', 2, 96, 48, 8, 16, 1, 2, 0, 1, ('wimg',), ((5, 1),), (Rec(0, 0, 0, STORE, 0, 0, 0, 1, 1, 1, 0, 0, 0),)),
    Row('f32_dgrad_stride2_factor_3x3', 'dgrad', 3, 72, 32, 12, 16, 3, 2, 1, 1, ('factor',), (), (Rec(0, 0, 4, FACTOR, 0, 0, 0, 2, 1, 4, 0, 0, 0),)),
    Row('f32_dgrad_stride2_factor_1x1_acc', 'dgrad', 2, 64, 32, 8, 16, 1, 2, 0, 1, ('factor', 'acc'), (), (Rec(0, 0, 4, FACTOR, 0, 0, 0, 1, 1, 1, 0, 0, 0),)),
    Row('rag_fwd_store_5x7_bias', 'fwd', 3, 32, 100, 5, 7, 3, 1, 1, 1, ('rag', 'bias'), (), (Rec(0, 0, 0, STORE, 0, 1, 0, 1, 1, 1, 0, 0, 0),)),
    Row('rag_fwd_store_9x9_acc', 'fwd', 2, 48, 99, 9, 9, 1, 1, 0, 1, ('rag', 'acc', 'wimg'), (), (Rec(0, 0, 0, STORE, 0, 1, 0, 2, 1, 1, 0, 0, 0),)),
    Row('rag_dgrad_store_9x9_acc', 'dgrad', 2, 100, 32, 9, 9, 3, 1, 1, 1, ('rag', 'acc'), (), (Rec(0, 0, 0, STORE, 0, 1, 0, 2, 1, 1, 0, 0, 0),)),
    Row('rag_dgrad_store_5x7', 'dgrad', 3, 200, 48, 5, 7, 1, 1, 0, 1, ('rag',), (), (Rec(0, 0, 0, STORE, 0, 1, 0, 2, 1, 1, 0, 0, 0),)),
    Row('rag_fwd_infer_9x9_bias_res_relu', 'fwd', 2, 32, 200, 9, 9, 3, 1, 1, 1, ('rag', 'infer', 'wimg', 'bias', 'res', 'relu'), (), (Rec(0, 0, 0, INFER, 0, 1, 0, 4, 1, 1, 0, 0, 0),)),
    Row('rag_fwd_infer_factor_5x7', 'fwd', 3, 32, 99, 5, 7, 3, 1, 1, 1, ('rag', 'infer', 'wimg', 'factor', 'bias', 'res', 'relu'), (), (Rec(0, 0, 4, INFER_FACTOR, 0, 1, 0, 1, 1, 1, 0, 0, 0),)),
    Row('rag_fwd_factor_5x7', 'fwd', 3, 32, 64, 5, 7, 3, 1, 1, 1, ('rag', 'factor'), (), (Rec(0, 0, 4, FACTOR, 0, 1, 0, 1, 1, 1, 0, 0, 0),)),
    Row('rag_dgrad_factor_9x9_acc', 'dgrad', 2, 72, 32, 9, 9, 3, 1, 1, 1, ('rag', 'factor', 'acc'), (), (Rec(0, 0, 4, FACTOR, 0, 1, 0, 2, 1, 1, 0, 0, 0),)),
    Row('rag_fwd_split2_roundup_bias_acc', 'fwd', 3, 64, 99, 5, 7, 1, 1, 0, 1, ('rag', 'bias', 'acc'), ((1, 2),), (Rec(0, 0, 0, STORE, 0, 1, 0, 1, 2, 1, 2, 4, 1),)),
    Row('rag_fwd_split4_uneven_infer_res_relu', 'fwd', 2, 32, 100, 9, 9, 3, 1, 1, 1, ('rag', 'infer', 'wimg', 'bias', 'res', 'relu'), ((1, 4),), (Rec(0, 0, 0, STORE, 0, 1, 0, 2, 4, 1, 5, 4, 1),)),
    Row('rag_fwd_split2_infer_factor', 'fwd', 3, 32, 99, 5, 7, 3, 1, 1, 1, ('rag', 'infer', 'wimg', 'factor', 'bias', 'res', 'relu'), ((1, 2),), (Rec(0, 0, 4, STORE, 0, 1, 0, 1, 2, 1, 9, 4, 1),)),
    Row('rag_fwd_split4_uneven_factor', 'fwd', 3, 32, 65, 5, 7, 3, 1, 1, 1, ('rag', 'factor'), ((1, 4),), (Rec(0, 0, 4, STORE, 0, 1, 0, 1, 4, 1, 5, 4, 1),)),
    Row('rag_dgrad_split2_factor_acc', 'dgrad', 2, 72, 32, 9, 9, 3, 1, 1, 1, ('rag', 'factor', 'acc'), ((1, 2),), (Rec(0, 0, 4, STORE, 0, 1, 0, 2, 2, 1, 9, 4, 1),)),
    Row('rag_img_fwd_store_5x7_bias', 'fwd', 3, 32, 112, 5, 7, 3, 1, 1, 1, ('rag', 'img', 'bias'), (), (Rec(0, 1, 0, STORE, 0, 1, 0, 1, 1, 1, 0, 0, 0),)),
    Row('rag_img_dgrad_store_9x9_acc', 'dgrad', 2, 96, 32, 9, 9, 3, 1, 1, 1, ('rag', 'img', 'acc', 'wimg'), (), (Rec(0, 1, 0, STORE, 0, 1, 0, 2, 1, 1, 0, 0, 0),)),
    Row('rag_img_fwd_split2', 'fwd', 3, 64, 99, 5, 7, 1, 1, 0, 1, ('rag', 'img'), ((1, 2),), (Rec(0, 1, 0, STORE, 0, 1, 0, 1, 2, 1, 2, 4, 1),)),
    Row('rag_img_fwd_tapi_planned_split', 'fwd', 1, 1024, 96, 5, 7, 3, 1, 1, 1, ('rag', 'img', 'long'), (), (Rec(0, 1, 0, STORE, 1, 1, 0, 1, 8, 1, 72, 4, 1),)),
    Row('rag_img_dgrad_tapi_unsplit', 'dgrad', 1, 96, 1024, 5, 7, 3, 1, 1, 1, ('rag', 'img', 'long'), ((1, 1),), (Rec(0, 1, 0, STORE, 1, 1, 0, 1, 1, 1, 0, 0, 0),)),
    Row('img_fwd_store_200_bias', 'fwd', 3, 32, 200, 12, 12, 1, 1, 0, 1, ('img', 'bias', 'wimg'), (), (Rec(0, 1, 0, STORE, 0, 0, 0, 8, 1, 1, 0, 0, 0),)),
    Row('img_fwd_store_320_stride2', 'fwd', 2, 32, 320, 8, 16, 3, 2, 1, 1, ('img', 'acc'), (), (Rec(0, 1, 0, STORE, 0, 0, 0, 3, 1, 1, 0, 0, 0),)),
    Row('img_dgrad_store_stride2_3x3', 'dgrad', 3, 128, 32, 12, 16, 3, 2, 1, 1, ('img',), (), (Rec(0, 1, 0, STORE, 0, 0, 0, 2, 1, 4, 0, 0, 0),)),
    Row('img_fwd_stats_320_3x3', 'fwd', 3, 32, 320, 12, 12, 3, 1, 1, 1, ('img', 'sums'), (), (Rec(0, 1, 0, STATS, 0, 0, 0, 12, 1, 1, 0, 0, 0),)),
    Row('img_dgrad_bwdsums_200', 'dgrad', 3, 200, 32, 12, 12, 1, 1, 0, 1, ('img', 'sums'), (), (Rec(0, 1, 0, BWD_SUMS, 0, 0, 0, 8, 1, 1, 0, 0, 0),)),
    Row('img_dgrad_accsrc_200', 'dgrad', 2, 200, 32, 8, 12, 3, 1, 1, 1, ('img', 'accsrc'), (), (Rec(0, 1, 0, STORE, 0, 0, 0, 4, 1, 1, 0, 0, 0),)),
    Row('img_fwd_factor_128', 'fwd', 3, 32, 128, 12, 12, 3, 1, 1, 1, ('img', 'factor'), (), (Rec(0, 1, 0, FACTOR_IMG, 0, 0, 0, 4, 1, 1, 0, 0, 0),)),
    Row('img_dgrad_factor_200_acc', 'dgrad', 2, 200, 32, 8, 12, 3, 1, 1, 1, ('img', 'factor', 'acc'), (), (Rec(0, 1, 0, FACTOR_IMG, 0, 0, 0, 4, 1, 1, 0, 0, 0),)),
    Row('img_fwd_factor_stats_128', 'fwd', 3, 32, 128, 12, 12, 3, 1, 1, 1, ('img', 'factor', 'sums'), (), (Rec(0, 1, 0, FACTOR_STATS, 0, 0, 0, 4, 1, 1, 0, 0, 0),)),
    Row('img_dgrad_factor_bwdsums_200', 'dgrad', 3, 200, 32, 12, 12, 1, 1, 0, 1, ('img', 'factor', 'sums'), (), (Rec(0, 1, 0, FACTOR_BWD_SUMS, 0, 0, 0, 8, 1, 1, 0, 0, 0),)),
    Row('img_fwd_infer_128_bias_res_relu', 'fwd', 3, 32, 128, 12, 12, 3, 1, 1, 1, ('img', 'infer', 'wimg', 'bias', 'res', 'relu'), (), (Rec(0, 1, 0, INFER, 0, 0, 0, 4, 1, 1, 0, 0, 0),)),
    Row('img_fwd_split2_stats_200', 'fwd', 3, 64, 200, 12, 12, 1, 1, 0, 1, ('img', 'sums'), ((1, 2),), (Rec(0, 1, 0, STORE, 0, 0, 0, 8, 2, 1, 2, 2, 3),)),
    Row('img_dgrad_split2_factor_bwdsums_n18', 'dgrad', 18, 128, 32, 4, 4, 1, 1, 0, 1, ('img', 'factor', 'sums'), ((1, 2),), (Rec(0, 1, 0, STORE, 0, 0, 0, 3, 2, 1, 1, 3, 16),)),
    Row('img_fwd_tapi_store_planned_split', 'fwd', 1, 1024, 128, 8, 8, 3, 1, 1, 1, ('img', 'long', 'bias'), (), (Rec(0, 1, 0, STORE, 1, 0, 0, 1, 8, 1, 72, 1, 1),)),
    Row('img_fwd_tapi_store_unsplit', 'fwd', 1, 1024, 128, 8, 8, 3, 1, 1, 1, ('img', 'long', 'wimg'), ((1, 1),), (Rec(0, 1, 0, STORE, 1, 0, 0, 1, 1, 1, 0, 0, 0),)),
    Row('img_fwd_tapi_stats', 'fwd', 1, 1024, 128, 8, 8, 3, 1, 1, 1, ('img', 'long', 'sums'), ((1, 1),), (Rec(0, 1, 0, STATS, 1, 0, 0, 1, 1, 1, 0, 0, 0),)),
    Row('img_dgrad_tapi_bwdsums', 'dgrad', 1, 128, 1024, 8, 8, 3, 1, 1, 1, ('img', 'long', 'sums'), ((1, 1),), (Rec(0, 1, 0, BWD_SUMS, 1, 0, 0, 1, 1, 1, 0, 0, 0),)),
    Row('rows_fwd_store_200_bias', 'fwd', 3, 32, 200, 12, 12, 1, 1, 0, 1, ('rows', 'bias'), (), (Rec(0, 1, 0, STORE, 0, 0, 1, 8, 1, 1, 0, 0, 0),)),
    Row('rows_dgrad_store_stride2_3x3', 'dgrad', 3, 128, 32, 12, 16, 3, 2, 1, 1, ('rows', 'acc'), (), (Rec(0, 1, 0, STORE, 0, 0, 1, 2, 1, 4, 0, 0, 0),)),
    Row('rows_fwd_stats_320_3x3', 'fwd', 3, 32, 320, 12, 12, 3, 1, 1, 1, ('rows', 'sums', 'wimg'), (), (Rec(0, 1, 0, STATS, 0, 0, 1, 12, 1, 1, 0, 0, 0),)),
    Row('rows_dgrad_bwdsums_200', 'dgrad', 3, 200, 32, 12, 12, 3, 1, 1, 1, ('rows', 'sums'), (), (Rec(0, 1, 0, BWD_SUMS, 0, 0, 1, 8, 1, 1, 0, 0, 0),)),
    Row('rows_dgrad_accsrc_mask_128', 'dgrad', 2, 128, 48, 8, 12, 1, 1, 0, 1, ('rows', 'accsrc', 'accmask'), (), (Rec(0, 1, 0, STORE, 0, 0, 1, 2, 1, 1, 0, 0, 0),)),
    Row('rows_fwd_split2_stats_n18', 'fwd', 18, 64, 128, 4, 4, 1, 1, 0, 1, ('rows', 'sums'), ((1, 2),), (Rec(0, 1, 0, STORE, 0, 0, 1, 3, 2, 1, 2, 2, 16),)),
    Row('rows_fwd_tapi_store_planned_split', 'fwd', 1, 1024, 128, 8, 8, 3, 1, 1, 1, ('rows', 'long'), (), (Rec(0, 1, 0, STORE, 1, 0, 1, 1, 8, 1, 72, 1, 1),)),
    Row('rows_dgrad_tapi_store_unsplit', 'dgrad', 1, 128, 1024, 8, 8, 3, 1, 1, 1, ('rows', 'long'), ((1, 1),), (Rec(0, 1, 0, STORE, 1, 0, 1, 1, 1, 1, 0, 0, 0),)),
    Row('rows_fwd_tapi_stats', 'fwd', 1, 1024, 128, 8, 8, 3, 1, 1, 1, ('rows', 'long', 'sums'), ((1, 1),), (Rec(0, 1, 0, STATS, 1, 0, 1, 1, 1, 1, 0, 0, 0),)),
    Row('rows_dgrad_tapi_bwdsums', 'dgrad', 1, 128, 1024, 8, 8, 3, 1, 1, 1, ('rows', 'long', 'sums'), ((1, 1),), (Rec(0, 1, 0, BWD_SUMS, 1, 0, 1, 1, 1, 1, 0, 0, 0),)),
    Row('x96_fwd_store_80_bias', 'fwd', 3, 32, 80, 12, 12, 3, 1, 1, 1, ('img', 'bias'), (), (Rec(96, 1, 0, STORE, 0, 0, 0, 4, 1, 1, 0, 0, 0),)),
    Row('x96_dgrad_store_272_stride2', 'dgrad', 2, 272, 32, 8, 16, 3, 2, 1, 1, ('img', 'wimg'), (), (Rec(96, 1, 0, STORE, 0, 0, 0, 3, 1, 4, 0, 0, 0),)),
    Row('x96_dgrad_store_144_stride2_1x1_class_launches', 'dgrad', 3, 144, 32, 12, 16, 1, 2, 0, 1, ('img',), ((5, 1),), (Rec(96, 1, 0, STORE, 0, 0, 0, 4, 1, 1, 0, 0, 0),)),
    Row('x96_fwd_stats_144', 'fwd', 3, 32, 144, 12, 12, 1, 1, 0, 1, ('img', 'sums', 'bias'), (), (Rec(96, 1, 0, STATS, 0, 0, 0, 8, 1, 1, 0, 0, 0),)),
    Row('x96_fwd_stats_272_w4', 'fwd', 7, 32, 272, 6, 4, 3, 1, 1, 1, ('img', 'sums'), (), (Rec(96, 1, 0, STATS, 0, 0, 0, 6, 1, 1, 0, 0, 0),)),
    Row('x96_dgrad_bwdsums_272', 'dgrad', 3, 272, 32, 12, 12, 1, 1, 0, 1, ('img', 'sums', 'wimg'), (), (Rec(96, 1, 0, BWD_SUMS, 0, 0, 0, 12, 1, 1, 0, 0, 0),)),
    Row('x96_dgrad_bwdsums_80_3x3', 'dgrad', 2, 80, 48, 8, 12, 3, 1, 1, 1, ('img', 'sums', 'wimg'), (), (Rec(96, 1, 0, BWD_SUMS, 0, 0, 0, 2, 1, 1, 0, 0, 0),)),
    Row('x96_fwd_infer_80_bias_res_relu', 'fwd', 3, 32, 80, 12, 12, 3, 1, 1, 1, ('img', 'infer', 'wimg', 'bias', 'res', 'relu'), (), (Rec(96, 1, 0, INFER, 0, 0, 0, 4, 1, 1, 0, 0, 0),)),
    Row('x96_fwd_infer_272_acc', 'fwd', 2, 32, 272, 8, 8, 1, 1, 0, 1, ('img', 'infer', 'wimg', 'bias', 'acc'), (), (Rec(96, 1, 0, INFER, 0, 0, 0, 3, 1, 1, 0, 0, 0),)),
    Row('x96_fwd_factor_144', 'fwd', 3, 32, 144, 12, 12, 3, 1, 1, 1, ('img', 'factor'), (), (Rec(96, 1, 0, STORE, 0, 0, 0, 8, 1, 1, 0, 0, 0),)),
    Row('x96_fwd_factor_stats_80', 'fwd', 3, 32, 80, 12, 12, 3, 1, 1, 1, ('img', 'factor', 'sums'), (), (Rec(96, 1, 0, STATS, 0, 0, 0, 4, 1, 1, 0, 0, 0),)),
    Row('x96_dgrad_factor_bwdsums_144', 'dgrad', 3, 144, 32, 12, 12, 3, 1, 1, 1, ('img', 'factor', 'sums'), (), (Rec(96, 1, 0, BWD_SUMS, 0, 0, 0, 8, 1, 1, 0, 0, 0),)),
    Row('x96_dgrad_accsrc_mask_272', 'dgrad', 2, 272, 32, 8, 12, 1, 1, 0, 1, ('img', 'accsrc', 'accmask'), (), (Rec(96, 1, 0, STORE, 0, 0, 0, 6, 1, 1, 0, 0, 0),)),
    Row('x96_fwd_split4_uneven_stats_n3', 'fwd', 3, 32, 144, 12, 12, 3, 1, 1, 1, ('img', 'sums', 'bias'), ((1, 4),), (Rec(96, 1, 0, STORE, 0, 0, 0, 8, 4, 1, 5, 2, 3),)),
    Row('x96_dgrad_split2_bwdsums_n18', 'dgrad', 18, 80, 32, 4, 4, 1, 1, 0, 1, ('img', 'sums'), ((1, 2),), (Rec(96, 1, 0, STORE, 0, 0, 0, 3, 2, 1, 1, 3, 16),)),
    Row('x96_fwd_tapi_store_planned_split', 'fwd', 1, 1024, 80, 8, 8, 3, 1, 1, 1, ('img', 'long'), (), (Rec(96, 1, 0, STORE, 1, 0, 0, 1, 8, 1, 72, 1, 1),)),
    Row('x96_dgrad_tapi_store_unsplit', 'dgrad', 1, 144, 1024, 8, 8, 3, 1, 1, 1, ('img', 'long'), ((1, 1),), (Rec(96, 1, 0, STORE, 1, 0, 0, 2, 1, 1, 0, 0, 0),)),
    Row('x96_fwd_tapi_stats_144', 'fwd', 1, 1024, 144, 8, 8, 3, 1, 1, 1, ('img', 'long', 'sums'), ((1, 1),), (Rec(96, 1, 0, STATS, 1, 0, 0, 2, 1, 1, 0, 0, 0),)),
    Row('x96_dgrad_tapi_bwdsums_80', 'dgrad', 1, 80, 1024, 8, 8, 3, 1, 1, 1, ('img', 'long', 'sums'), ((1, 1),), (Rec(96, 1, 0, BWD_SUMS, 1, 0, 0, 1, 1, 1, 0, 0, 0),)),
    Row('x96_rows_fwd_store_144', 'fwd', 3, 32, 144, 12, 12, 3, 1, 1, 1, ('rows', 'acc'), (), (Rec(96, 1, 0, STORE, 0, 0, 1, 8, 1, 1, 0, 0, 0),)),
    Row('x96_rows_fwd_stats_80', 'fwd', 3, 32, 80, 12, 12, 1, 1, 0, 1, ('rows', 'sums'), (), (Rec(96, 1, 0, STATS, 0, 0, 1, 4, 1, 1, 0, 0, 0),)),
    Row('x96_rows_dgrad_bwdsums_272', 'dgrad', 2, 272, 32, 8, 12, 3, 1, 1, 1, ('rows', 'sums'), (), (Rec(96, 1, 0, BWD_SUMS, 0, 0, 1, 6, 1, 1, 0, 0, 0),)),
    Row('x96_rows_fwd_tapi_store_planned_split', 'fwd', 1, 1024, 80, 8, 8, 3, 1, 1, 1, ('rows', 'long'), (), (Rec(96, 1, 0, STORE, 1, 0, 1, 1, 8, 1, 72, 1, 1),)),
    Row('x96_rows_fwd_tapi_store_unsplit', 'fwd', 1, 1024, 144, 8, 8, 3, 1, 1, 1, ('rows', 'long', 'bias'), ((1, 1),), (Rec(96, 1, 0, STORE, 1, 0, 1, 2, 1, 1, 0, 0, 0),)),
    Row('x96_rows_fwd_tapi_stats_80', 'fwd', 1, 1024, 80, 8, 8, 3, 1, 1, 1, ('rows', 'long', 'sums'), ((1, 1),), (Rec(96, 1, 0, STATS, 1, 0, 1, 1, 1, 1, 0, 0, 0),)),
    Row('x96_rows_dgrad_tapi_bwdsums_144', 'dgrad', 1, 144, 1024, 8, 8, 3, 1, 1, 1, ('rows', 'long', 'sums'), ((1, 1),), (Rec(96, 1, 0, BWD_SUMS, 1, 0, 1, 2, 1, 1, 0, 0, 0),)),
    Row('x64_fwd_store_48_bias', 'fwd', 3, 32, 48, 12, 12, 3, 1, 1, 1, ('img', 'bias'), (), (Rec(64, 1, 0, STORE, 0, 0, 0, 4, 1, 1, 0, 0, 0),)),
    Row('x64_dgrad_store_64_stride2', 'dgrad', 3, 64, 32, 12, 16, 3, 2, 1, 1, ('img', 'acc'), (), (Rec(64, 1, 0, STORE, 0, 0, 0, 2, 1, 4, 0, 0, 0),)),
    Row('x64_fwd_stats_48', 'fwd', 3, 32, 48, 12, 12, 1, 1, 0, 1, ('img', 'sums'), (), (Rec(64, 1, 0, STATS, 0, 0, 0, 4, 1, 1, 0, 0, 0),)),
    Row('x64_dgrad_bwdsums_48', 'dgrad', 3, 48, 32, 12, 12, 3, 1, 1, 1, ('img', 'sums'), (), (Rec(64, 1, 0, BWD_SUMS, 0, 0, 0, 4, 1, 1, 0, 0, 0),)),
    Row('x64_fwd_infer_64_bias_res_relu', 'fwd', 2, 32, 64, 8, 12, 3, 1, 1, 1, ('img', 'infer', 'wimg', 'bias', 'res', 'relu'), (), (Rec(64, 1, 0, INFER, 0, 0, 0, 2, 1, 1, 0, 0, 0),)),
    Row('x64_fwd_factor_stats_64', 'fwd', 3, 32, 64, 12, 12, 3, 1, 1, 1, ('img', 'factor', 'sums'), (), (Rec(64, 1, 0, STATS, 0, 0, 0, 4, 1, 1, 0, 0, 0),)),
    Row('x64_dgrad_factor_64_acc', 'dgrad', 2, 64, 32, 8, 12, 3, 1, 1, 1, ('img', 'factor', 'acc'), (), (Rec(64, 1, 0, STORE, 0, 0, 0, 2, 1, 1, 0, 0, 0),)),
    Row('x64_fwd_split2_store_48', 'fwd', 3, 64, 48, 12, 12, 1, 1, 0, 1, ('img', 'bias'), ((1, 2),), (Rec(64, 1, 0, STORE, 0, 0, 0, 4, 2, 1, 2, 1, 3),)),
    Row('x64_fwd_tapi_falls_back_to_tap_outer', 'fwd', 1, 1024, 64, 8, 8, 3, 1, 1, 1, ('img', 'long'), ((1, 1),), (Rec(64, 1, 0, STORE, 0, 0, 0, 1, 1, 1, 0, 0, 0),)),
    Row('x64_rows_fwd_store_64', 'fwd', 2, 32, 64, 8, 8, 3, 1, 1, 1, ('rows', 'bias'), (), (Rec(64, 1, 0, STORE, 0, 0, 1, 1, 1, 1, 0, 0, 0),)),
    Row('x64_rows_fwd_stats_48', 'fwd', 3, 32, 48, 12, 12, 3, 1, 1, 1, ('rows', 'sums'), (), (Rec(64, 1, 0, STATS, 0, 0, 1, 4, 1, 1, 0, 0, 0),)),
    Row('x64_rows_dgrad_bwdsums_48', 'dgrad', 3, 48, 32, 12, 12, 1, 1, 0, 1, ('rows', 'sums'), (), (Rec(64, 1, 0, BWD_SUMS, 0, 0, 1, 4, 1, 1, 0, 0, 0),)),
]
