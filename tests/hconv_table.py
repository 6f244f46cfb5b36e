"""The cases of tests/test_hconv_paths_gpu.py and tests/test_hconv_paths_host.py: one literal row per call of the fp16 convolution entries of csrc/p3d_hconv.hip
(hconv_gather_kernel<32, EPI 0..4>, hconv_wgrad_kernel, hwgrad_reduce_kernel) that must take one named path through them, at the smallest shape that reaches it.

A row is the entry, the descriptor (square filters: N C H W K R stride pad dil) and the options; PATHS holds, per row, the path the call is expected to take, written
out.  The path is DERIVED here as well, by restating four pieces of the library's host code -- launch_gather's choice of EPI, the narrow wave layout (M <= 64),
fill_class_h and hwgrad_plan -- and the host test holds the two to each other, the restatements to the library (the workspace query, p3d_hconv2d_sum_rows) and the
set of paths to REQUIRED, so that a row cannot be dropped or moved off its path without a failure.  No GPU, no torch and no library needed to import this.

Entries: 'fwd' p3d_hconv2d_fwd, 'stats' p3d_hconv2d_fwd_stats, 'infer' p3d_hconv2d_fwd_infer, 'dgrad' p3d_hconv2d_dgrad, 'sums' p3d_hconv2d_dgrad_sums, 'wgrad' p3d_hconv2d_wgrad.
M is the result's channel count (K forward, C for a data gradient), Kc the reduction's (C forward, K for a data gradient).
Options: 'bias'; 'mask' (mask_in) and 'mult' of a partial convolution; 'res' / 'relu' (infer); 'acc' (d->accumulate: onto what dx / dw held); 'zpad' (a data gradient whose
channels 3.. are padding: zero weight rows); 'xmask' (wgrad's mask_in), 'creal3' / 'creal1' (c_real of d->C = 8), 'small' (scale 1/1024 instead of 1).
Path of a gather row: 'E<epi> narrow|wide m<row tiles> n<pixel tiles of the largest class> nk<K-steps of each pixel class, in grid.y order>', EPI 4 with 'p<passes of the
last row tile>'.  Path of a wgrad row: 's<splits> kc<kchunk> last<pixels of the last split> m<row tiles> n<column tiles>'."""
import collections

Row = collections.namedtuple('Row', 'name entry n c h w k r stride pad dil opts')

ENTRIES = ('fwd', 'stats', 'infer', 'dgrad', 'sums', 'wgrad')
OPTIONS = dict(fwd={'bias', 'mask', 'mult'}, stats=set(), infer={'bias', 'mask', 'mult', 'res', 'relu'}, dgrad={'acc', 'mask', 'zpad'}, sums=set(),
               wgrad={'acc', 'xmask', 'creal3', 'creal1', 'small'})
HMS = 4                                 # largest stride of the class tables
BK_CHUNKS = 4                           # 16-B chunks of a K-step (BK = 32 halves)
WGRAD_TARGET = 384                      # blocks hwgrad_plan aims at

ROWS = [
    # ---- every epilogue at every row-tile layout: M narrow (8, 40, 64), wide in one tile (72, 128), over two and three tiles with a ragged last one (136, 200, 272);
    #      3x3, Kc = 16 (18 chunks: 5 K-steps, the last with two dead chunks); 70 pixel columns, or 198 (a ragged second tile) ----
    Row('m8_bias', 'fwd', 2, 16, 5, 7, 8, 3, 1, 1, 1, ('bias',)),
    Row('m8_plain', 'fwd', 2, 16, 5, 7, 8, 3, 1, 1, 1, ()),
    Row('m8_stats', 'stats', 2, 16, 5, 7, 8, 3, 1, 1, 1, ()),
    Row('m8_sums', 'sums', 2, 8, 5, 7, 16, 3, 1, 1, 1, ()),
    Row('m8_infer', 'infer', 2, 16, 5, 7, 8, 3, 1, 1, 1, ('bias', 'res')),
    Row('m40_bias', 'fwd', 2, 16, 9, 11, 40, 3, 1, 1, 1, ('bias',)),
    Row('m40_plain', 'fwd', 2, 16, 9, 11, 40, 3, 1, 1, 1, ()),
    Row('m40_mult', 'fwd', 2, 16, 9, 11, 40, 3, 1, 1, 1, ('mult',)),
    Row('m40_stats', 'stats', 2, 16, 9, 11, 40, 3, 1, 1, 1, ()),
    Row('m40_sums', 'sums', 2, 40, 9, 11, 16, 3, 1, 1, 1, ()),
    Row('m40_infer', 'infer', 2, 16, 9, 11, 40, 3, 1, 1, 1, ('bias', 'res')),
    Row('m64_bias', 'fwd', 2, 16, 5, 7, 64, 3, 1, 1, 1, ('bias',)),
    Row('m64_plain', 'fwd', 2, 16, 5, 7, 64, 3, 1, 1, 1, ()),
    Row('m64_mult', 'fwd', 2, 16, 5, 7, 64, 3, 1, 1, 1, ('mult',)),
    Row('m64_stats', 'stats', 2, 16, 5, 7, 64, 3, 1, 1, 1, ()),
    Row('m64_sums', 'sums', 2, 64, 5, 7, 16, 3, 1, 1, 1, ()),
    Row('m64_infer', 'infer', 2, 16, 5, 7, 64, 3, 1, 1, 1, ('bias', 'res')),
    Row('m72_bias', 'fwd', 2, 16, 9, 11, 72, 3, 1, 1, 1, ('bias',)),
    Row('m72_plain', 'fwd', 2, 16, 9, 11, 72, 3, 1, 1, 1, ()),
    Row('m72_stats', 'stats', 2, 16, 9, 11, 72, 3, 1, 1, 1, ()),
    Row('m72_sums', 'sums', 2, 72, 9, 11, 16, 3, 1, 1, 1, ()),
    Row('m72_infer', 'infer', 2, 16, 9, 11, 72, 3, 1, 1, 1, ('bias', 'res')),
    Row('m128_bias', 'fwd', 2, 16, 5, 7, 128, 3, 1, 1, 1, ('bias',)),
    Row('m128_plain', 'fwd', 2, 16, 5, 7, 128, 3, 1, 1, 1, ()),
    Row('m128_stats', 'stats', 2, 16, 5, 7, 128, 3, 1, 1, 1, ()),
    Row('m128_sums', 'sums', 2, 128, 5, 7, 16, 3, 1, 1, 1, ()),
    Row('m128_infer', 'infer', 2, 16, 5, 7, 128, 3, 1, 1, 1, ('bias', 'res')),
    Row('m136_bias', 'fwd', 2, 16, 9, 11, 136, 3, 1, 1, 1, ('bias',)),
    Row('m136_plain', 'fwd', 2, 16, 9, 11, 136, 3, 1, 1, 1, ()),
    Row('m136_mult', 'fwd', 2, 16, 9, 11, 136, 3, 1, 1, 1, ('mult',)),
    Row('m136_stats', 'stats', 2, 16, 9, 11, 136, 3, 1, 1, 1, ()),
    Row('m136_sums', 'sums', 2, 136, 9, 11, 16, 3, 1, 1, 1, ()),
    Row('m136_infer', 'infer', 2, 16, 9, 11, 136, 3, 1, 1, 1, ('bias', 'res')),
    Row('m200_bias', 'fwd', 2, 16, 5, 7, 200, 3, 1, 1, 1, ('bias',)),
    Row('m200_plain', 'fwd', 2, 16, 5, 7, 200, 3, 1, 1, 1, ()),
    Row('m200_stats', 'stats', 2, 16, 5, 7, 200, 3, 1, 1, 1, ()),
    Row('m200_sums', 'sums', 2, 200, 5, 7, 16, 3, 1, 1, 1, ()),
    Row('m200_infer', 'infer', 2, 16, 5, 7, 200, 3, 1, 1, 1, ('bias', 'res')),
    Row('m272_bias', 'fwd', 2, 16, 9, 11, 272, 3, 1, 1, 1, ('bias',)),
    Row('m272_plain', 'fwd', 2, 16, 9, 11, 272, 3, 1, 1, 1, ()),
    Row('m272_stats', 'stats', 2, 16, 9, 11, 272, 3, 1, 1, 1, ()),
    Row('m272_sums', 'sums', 2, 272, 9, 11, 16, 3, 1, 1, 1, ()),
    Row('m272_infer', 'infer', 2, 16, 9, 11, 272, 3, 1, 1, 1, ('bias', 'res')),
    # ---- EPI 4: none / res / relu / both, bare and with mask_in + mult + bias, at M = 72 (two passes, the second with one live chunk), 200 (the second tile takes two
    #      passes) and 192 (the second tile takes one); 3x3, Kc = 8 ----
    Row('i72_none', 'infer', 2, 8, 9, 11, 72, 3, 1, 1, 1, ()),
    Row('i72_res', 'infer', 2, 8, 9, 11, 72, 3, 1, 1, 1, ('res',)),
    Row('i72_relu', 'infer', 2, 8, 9, 11, 72, 3, 1, 1, 1, ('relu',)),
    Row('i72_res_relu', 'infer', 2, 8, 9, 11, 72, 3, 1, 1, 1, ('res', 'relu')),
    Row('i72_all_none', 'infer', 2, 8, 9, 11, 72, 3, 1, 1, 1, ('bias', 'mask', 'mult')),
    Row('i72_all_res', 'infer', 2, 8, 9, 11, 72, 3, 1, 1, 1, ('bias', 'mask', 'mult', 'res')),
    Row('i72_all_relu', 'infer', 2, 8, 9, 11, 72, 3, 1, 1, 1, ('bias', 'mask', 'mult', 'relu')),
    Row('i72_all_res_relu', 'infer', 2, 8, 9, 11, 72, 3, 1, 1, 1, ('bias', 'mask', 'mult', 'res', 'relu')),
    Row('i200_none', 'infer', 2, 8, 9, 11, 200, 3, 1, 1, 1, ()),
    Row('i200_res', 'infer', 2, 8, 9, 11, 200, 3, 1, 1, 1, ('res',)),
    Row('i200_relu', 'infer', 2, 8, 9, 11, 200, 3, 1, 1, 1, ('relu',)),
    Row('i200_res_relu', 'infer', 2, 8, 9, 11, 200, 3, 1, 1, 1, ('res', 'relu')),
    Row('i200_all_none', 'infer', 2, 8, 9, 11, 200, 3, 1, 1, 1, ('bias', 'mask', 'mult')),
    Row('i200_all_res', 'infer', 2, 8, 9, 11, 200, 3, 1, 1, 1, ('bias', 'mask', 'mult', 'res')),
    Row('i200_all_relu', 'infer', 2, 8, 9, 11, 200, 3, 1, 1, 1, ('bias', 'mask', 'mult', 'relu')),
    Row('i200_all_res_relu', 'infer', 2, 8, 9, 11, 200, 3, 1, 1, 1, ('bias', 'mask', 'mult', 'res', 'relu')),
    Row('i192_none', 'infer', 2, 8, 9, 11, 192, 3, 1, 1, 1, ()),
    Row('i192_res', 'infer', 2, 8, 9, 11, 192, 3, 1, 1, 1, ('res',)),
    Row('i192_relu', 'infer', 2, 8, 9, 11, 192, 3, 1, 1, 1, ('relu',)),
    Row('i192_res_relu', 'infer', 2, 8, 9, 11, 192, 3, 1, 1, 1, ('res', 'relu')),
    Row('i192_all_none', 'infer', 2, 8, 9, 11, 192, 3, 1, 1, 1, ('bias', 'mask', 'mult')),
    Row('i192_all_res', 'infer', 2, 8, 9, 11, 192, 3, 1, 1, 1, ('bias', 'mask', 'mult', 'res')),
    Row('i192_all_relu', 'infer', 2, 8, 9, 11, 192, 3, 1, 1, 1, ('bias', 'mask', 'mult', 'relu')),
    Row('i192_all_res_relu', 'infer', 2, 8, 9, 11, 192, 3, 1, 1, 1, ('bias', 'mask', 'mult', 'res', 'relu')),
    # ---- pixel columns: exactly one full tile (2 x 8 x 8), and tiles that span images (5 images of 35 pixels: the first tile holds three whole ones and ends in the
    #      fourth) ----
    Row('cols128_bias', 'fwd', 2, 8, 8, 8, 72, 3, 1, 1, 1, ('bias',)),
    Row('cols128_plain', 'fwd', 2, 8, 8, 8, 72, 3, 1, 1, 1, ()),
    Row('cols128_stats', 'stats', 2, 8, 8, 8, 72, 3, 1, 1, 1, ()),
    Row('cols128_sums', 'sums', 2, 72, 8, 8, 8, 3, 1, 1, 1, ()),
    Row('cols128_infer', 'infer', 2, 8, 8, 8, 72, 3, 1, 1, 1, ('bias', 'res', 'relu')),
    Row('img3_bias', 'fwd', 5, 8, 5, 7, 72, 3, 1, 1, 1, ('bias',)),
    Row('img3_plain', 'fwd', 5, 8, 5, 7, 72, 3, 1, 1, 1, ()),
    Row('img3_stats', 'stats', 5, 8, 5, 7, 72, 3, 1, 1, 1, ()),
    Row('img3_sums', 'sums', 5, 72, 5, 7, 8, 3, 1, 1, 1, ()),
    Row('img3_infer', 'infer', 5, 8, 5, 7, 72, 3, 1, 1, 1, ('bias', 'res', 'relu')),
    # ---- the K loop: 1 step with dead chunks, 1 full, 2 (5 and 8 chunks), 3, 4, and longer odd and even ones; C8 = 1 (four taps a step), 3 and 5 (steps straddle taps) ----
    Row('k_1x1_c8', 'fwd', 2, 8, 9, 11, 72, 1, 1, 0, 1, ()),
    Row('k_1x1_c32', 'fwd', 2, 32, 9, 11, 72, 1, 1, 0, 1, ()),
    Row('k_1x1_c40', 'fwd', 2, 40, 9, 11, 72, 1, 1, 0, 1, ()),
    Row('k_1x1_c64', 'fwd', 2, 64, 9, 11, 72, 1, 1, 0, 1, ('bias',)),
    Row('k_3x3_c8', 'fwd', 2, 8, 9, 11, 72, 3, 1, 1, 1, ()),
    Row('k_1x1_c128', 'fwd', 2, 128, 9, 11, 72, 1, 1, 0, 1, ()),
    Row('k_3x3_c24', 'fwd', 2, 24, 9, 11, 72, 3, 1, 1, 1, ('bias',)),
    Row('k_3x3_c40', 'fwd', 2, 40, 9, 11, 72, 3, 1, 1, 1, ()),
    Row('k_7x7_c8', 'fwd', 2, 8, 9, 11, 72, 7, 1, 3, 1, ()),
    Row('ki_1x1_c8', 'infer', 2, 8, 9, 11, 72, 1, 1, 0, 1, ('bias',)),
    Row('ki_3x3_c24', 'infer', 2, 24, 9, 11, 72, 3, 1, 1, 1, ('res',)),
    Row('kd_1x1_k8', 'dgrad', 2, 72, 9, 11, 8, 1, 1, 0, 1, ()),
    Row('kd_1x1_k40', 'dgrad', 2, 72, 9, 11, 40, 1, 1, 0, 1, ()),
    Row('kd_3x3_k8', 'dgrad', 2, 72, 9, 11, 8, 3, 1, 1, 1, ()),
    Row('kd_3x3_k8_acc', 'dgrad', 2, 72, 9, 11, 8, 3, 1, 1, 1, ('acc',)),
    Row('kd_3x3_k8_mask', 'dgrad', 2, 72, 9, 11, 8, 3, 1, 1, 1, ('mask',)),
    Row('kd_3x3_k8_both', 'dgrad', 2, 72, 9, 11, 8, 3, 1, 1, 1, ('acc', 'mask')),
    Row('kd_3x3_k24', 'dgrad', 2, 72, 9, 11, 24, 3, 1, 1, 1, ()),
    Row('kd_3x3_k40', 'dgrad', 2, 72, 9, 11, 40, 3, 1, 1, 1, ()),
    # ---- forward geometry: stride 1 to 4, dilation 2 and 4, 7x7 pad 3, no padding, H < W and H > W ----
    Row('g_s2', 'fwd', 2, 16, 13, 17, 40, 3, 2, 1, 1, ()),
    Row('g_s2_stats', 'stats', 2, 16, 17, 13, 40, 3, 2, 1, 1, ()),
    Row('g_s3', 'fwd', 2, 16, 17, 13, 40, 3, 3, 1, 1, ('bias',)),
    Row('g_s4', 'fwd', 2, 16, 14, 19, 40, 3, 4, 1, 1, ('mask', 'mult')),
    Row('g_s4_1x1', 'fwd', 2, 16, 18, 13, 40, 1, 4, 0, 1, ()),
    Row('g_d2', 'fwd', 2, 16, 11, 14, 40, 3, 1, 2, 2, ('bias',)),
    Row('g_d4', 'fwd', 2, 16, 14, 11, 40, 3, 1, 4, 4, ()),
    Row('g_p0', 'fwd', 2, 16, 11, 14, 40, 3, 1, 0, 1, ()),
    Row('g_7x7', 'fwd', 2, 8, 9, 12, 40, 7, 1, 3, 1, ('mask', 'mult', 'bias')),
    Row('g_7x7s2', 'infer', 2, 8, 17, 12, 40, 7, 2, 3, 1, ('bias', 'relu')),
    Row('g_s3_5x5', 'stats', 2, 8, 16, 19, 40, 5, 3, 2, 1, ()),
    Row('g_s2d2', 'infer', 2, 16, 15, 12, 40, 3, 2, 2, 2, ('res',)),
    # ---- the pixel classes of a strided data gradient, each plain, accumulating, with mask_in and with both (EPI 1, 1, 1, 0).  H and W are no multiples of the stride
    #      and the largest class has more column tiles than the smallest (143 against 120 or 100 columns) ----
    Row('d_3x3s2p1', 'dgrad', 1, 72, 25, 21, 16, 3, 2, 1, 1, ()),
    Row('d_3x3s2p1_acc', 'dgrad', 1, 72, 25, 21, 16, 3, 2, 1, 1, ('acc',)),
    Row('d_3x3s2p1_mask', 'dgrad', 1, 72, 25, 21, 16, 3, 2, 1, 1, ('mask',)),
    Row('d_3x3s2p1_both', 'dgrad', 1, 72, 25, 21, 16, 3, 2, 1, 1, ('acc', 'mask')),
    Row('d_3x3s2p1_zpad', 'dgrad', 1, 8, 25, 21, 16, 3, 2, 1, 1, ('zpad',)),
    Row('d_3x3s2p1_zpad_acc', 'dgrad', 1, 8, 25, 21, 16, 3, 2, 1, 1, ('acc', 'zpad')),
    Row('d_1x1s2', 'dgrad', 1, 8, 25, 21, 24, 1, 2, 0, 1, ()),
    Row('d_1x1s2_acc', 'dgrad', 1, 8, 25, 21, 24, 1, 2, 0, 1, ('acc',)),
    Row('d_1x1s2_mask', 'dgrad', 1, 8, 25, 21, 24, 1, 2, 0, 1, ('mask',)),
    Row('d_1x1s2_both', 'dgrad', 1, 8, 25, 21, 24, 1, 2, 0, 1, ('acc', 'mask')),
    Row('d_7x7s2p3', 'dgrad', 1, 64, 25, 21, 8, 7, 2, 3, 1, ()),
    Row('d_7x7s2p3_acc', 'dgrad', 1, 64, 25, 21, 8, 7, 2, 3, 1, ('acc',)),
    Row('d_7x7s2p3_mask', 'dgrad', 1, 64, 25, 21, 8, 7, 2, 3, 1, ('mask',)),
    Row('d_7x7s2p3_both', 'dgrad', 1, 64, 25, 21, 8, 7, 2, 3, 1, ('acc', 'mask')),
    Row('d_3x3s2p2d2', 'dgrad', 1, 136, 25, 21, 8, 3, 2, 2, 2, ()),
    Row('d_3x3s2p2d2_acc', 'dgrad', 1, 136, 25, 21, 8, 3, 2, 2, 2, ('acc',)),
    Row('d_3x3s2p2d2_mask', 'dgrad', 1, 136, 25, 21, 8, 3, 2, 2, 2, ('mask',)),
    Row('d_3x3s2p2d2_both', 'dgrad', 1, 136, 25, 21, 8, 3, 2, 2, 2, ('acc', 'mask')),
    Row('d_3x3s3p1', 'dgrad', 1, 40, 37, 31, 16, 3, 3, 1, 1, ()),
    Row('d_3x3s3p1_acc', 'dgrad', 1, 40, 37, 31, 16, 3, 3, 1, 1, ('acc',)),
    Row('d_3x3s3p1_mask', 'dgrad', 1, 40, 37, 31, 16, 3, 3, 1, 1, ('mask',)),
    Row('d_3x3s3p1_both', 'dgrad', 1, 40, 37, 31, 16, 3, 3, 1, 1, ('acc', 'mask')),
    Row('d_5x5s3p2', 'dgrad', 1, 128, 37, 31, 8, 5, 3, 2, 1, ()),
    Row('d_5x5s3p2_acc', 'dgrad', 1, 128, 37, 31, 8, 5, 3, 2, 1, ('acc',)),
    Row('d_5x5s3p2_mask', 'dgrad', 1, 128, 37, 31, 8, 5, 3, 2, 1, ('mask',)),
    Row('d_5x5s3p2_both', 'dgrad', 1, 128, 37, 31, 8, 5, 3, 2, 1, ('acc', 'mask')),
    Row('d_3x3s3p0d2', 'dgrad', 1, 200, 37, 31, 8, 3, 3, 0, 2, ()),
    Row('d_3x3s3p0d2_acc', 'dgrad', 1, 200, 37, 31, 8, 3, 3, 0, 2, ('acc',)),
    Row('d_3x3s3p0d2_mask', 'dgrad', 1, 200, 37, 31, 8, 3, 3, 0, 2, ('mask',)),
    Row('d_3x3s3p0d2_both', 'dgrad', 1, 200, 37, 31, 8, 3, 3, 0, 2, ('acc', 'mask')),
    Row('d_1x1s4', 'dgrad', 1, 272, 49, 41, 8, 1, 4, 0, 1, ()),
    Row('d_1x1s4_acc', 'dgrad', 1, 272, 49, 41, 8, 1, 4, 0, 1, ('acc',)),
    Row('d_1x1s4_mask', 'dgrad', 1, 272, 49, 41, 8, 1, 4, 0, 1, ('mask',)),
    Row('d_1x1s4_both', 'dgrad', 1, 272, 49, 41, 8, 1, 4, 0, 1, ('acc', 'mask')),
    Row('d_3x3s4p1', 'dgrad', 1, 72, 49, 41, 24, 3, 4, 1, 1, ()),
    Row('d_3x3s4p1_acc', 'dgrad', 1, 72, 49, 41, 24, 3, 4, 1, 1, ('acc',)),
    Row('d_3x3s4p1_mask', 'dgrad', 1, 72, 49, 41, 24, 3, 4, 1, 1, ('mask',)),
    Row('d_3x3s4p1_both', 'dgrad', 1, 72, 49, 41, 24, 3, 4, 1, 1, ('acc', 'mask')),
    Row('d_7x7s4p3', 'dgrad', 1, 8, 49, 41, 8, 7, 4, 3, 1, ()),
    Row('d_7x7s4p3_acc', 'dgrad', 1, 8, 49, 41, 8, 7, 4, 3, 1, ('acc',)),
    Row('d_7x7s4p3_mask', 'dgrad', 1, 8, 49, 41, 8, 7, 4, 3, 1, ('mask',)),
    Row('d_7x7s4p3_both', 'dgrad', 1, 8, 49, 41, 8, 7, 4, 3, 1, ('acc', 'mask')),
    # ---- weight gradient: the plans of WGRAD_PLANS, the reduce kernel's two loops alone and together (9, 32, 33, 40 splits) with accumulate 0 and 1, Wo = 1,
    #      strides, dilation, mask_in, c_real and scale ----
    Row('w_tiny', 'wgrad', 1, 8, 5, 3, 8, 1, 1, 0, 1, ()),
    Row('w_1x1', 'wgrad', 2, 64, 16, 16, 128, 1, 1, 0, 1, ()),
    Row('w_c24', 'wgrad', 2, 24, 17, 16, 72, 3, 1, 1, 1, ()),
    Row('w_7x7', 'wgrad', 1, 8, 33, 32, 64, 7, 1, 3, 1, ('small',)),
    Row('w_s9', 'wgrad', 1, 16, 48, 47, 64, 3, 1, 1, 1, ()),
    Row('w_s9_acc', 'wgrad', 1, 16, 48, 47, 64, 3, 1, 1, 1, ('acc',)),
    Row('w_s32', 'wgrad', 1, 8, 90, 90, 16, 3, 1, 1, 1, ()),
    Row('w_s32_acc', 'wgrad', 1, 8, 90, 90, 16, 3, 1, 1, 1, ('acc', 'small')),
    Row('w_s33', 'wgrad', 3, 16, 53, 53, 64, 3, 1, 1, 1, ()),
    Row('w_s33_acc', 'wgrad', 3, 16, 53, 53, 64, 3, 1, 1, 1, ('acc',)),
    Row('w_s40', 'wgrad', 1, 8, 100, 100, 40, 3, 1, 1, 1, ()),
    Row('w_s40_acc', 'wgrad', 1, 8, 100, 100, 40, 3, 1, 1, 1, ('acc', 'small')),
    Row('w_s64', 'wgrad', 2, 40, 96, 96, 136, 3, 1, 1, 1, ()),
    Row('w_s65', 'wgrad', 4, 8, 64, 65, 8, 1, 1, 0, 1, ('acc',)),
    Row('w_wo1', 'wgrad', 3, 8, 40, 1, 8, 3, 1, 1, 1, ()),
    Row('w_s2', 'wgrad', 2, 16, 21, 19, 40, 3, 2, 1, 1, ()),
    Row('w_s3', 'wgrad', 2, 16, 22, 20, 40, 3, 3, 1, 1, ('acc',)),
    Row('w_d2', 'wgrad', 2, 16, 13, 15, 40, 3, 1, 2, 2, ()),
    Row('w_xmask', 'wgrad', 2, 16, 20, 20, 64, 3, 1, 1, 1, ('xmask',)),
    Row('w_xmask_s2', 'wgrad', 2, 8, 33, 31, 72, 3, 2, 1, 1, ('xmask', 'acc')),
    Row('w_creal3', 'wgrad', 2, 8, 33, 31, 64, 7, 2, 3, 1, ('creal3',)),
    Row('w_creal3_acc', 'wgrad', 2, 8, 33, 31, 64, 7, 2, 3, 1, ('creal3', 'acc', 'small')),
    Row('w_creal1', 'wgrad', 1, 8, 33, 31, 64, 7, 2, 3, 1, ('creal1', 'xmask')),
]

# the weight-gradient plans the table must hold, worked out by hand from hwgrad_plan: (N, C, K, R, Ho, Wo) -> (splits, kchunk, pixels of the last split)
WGRAD_PLANS = {
    (1, 8, 8, 1, 5, 3): (1, 32, 15),
    (2, 64, 128, 1, 16, 16): (2, 256, 256),
    (2, 24, 72, 3, 17, 16): (3, 192, 160),
    (1, 8, 64, 7, 33, 32): (5, 224, 160),
    (1, 16, 64, 3, 48, 47): (9, 256, 208),
    (3, 16, 64, 3, 53, 53): (33, 256, 235),
    (1, 8, 40, 3, 100, 100): (40, 256, 16),
    (2, 40, 136, 3, 96, 96): (64, 288, 288),
    (4, 8, 8, 1, 64, 65): (65, 256, 256),
}


def ceil_div(a, b):
    return -(-a // b)


def conv_out(h, k, stride, pad, dil):
    return (h + 2 * pad - dil * (k - 1) - 1) // stride + 1


def out_hw(row):
    return conv_out(row.h, row.r, row.stride, row.pad, row.dil), conv_out(row.w, row.r, row.stride, row.pad, row.dil)


# ---- launch_gather: bias, and a factor on an accumulating launch, keep the single rounding of EPI 0; everything else plain goes through LDS (EPI 1) ----
def epi_of(row):
    o = set(row.opts)
    if row.entry in ('stats', 'sums', 'infer'):
        return dict(stats=2, sums=3, infer=4)[row.entry]
    bias = 'bias' in o
    dscale = ('mult' in o) if row.entry == 'fwd' else ('mask' in o)
    accumulate = row.entry == 'dgrad' and 'acc' in o
    return 1 if (not bias and not (dscale and accumulate)) else 0


def fill_class_h(par, R, stride, pad, dil):
    """(r0, step, n, off0, offstep) of pixel class `par`: its taps are r0 + step * j, j < n, and tap j reads the row i + off0 - offstep * j of dy for the class's row i"""
    first = second = -1
    n = 0
    for r in range(R):
        if (par + pad - r * dil) % stride != 0:
            continue
        if first < 0:
            first = r
        elif second < 0:
            second = r
        n += 1
    if first < 0:
        return 0, 1, 0, 0, 0
    step = 1 if second < 0 else second - first
    t0 = par + pad - first * dil
    off0 = t0 // stride if t0 >= 0 else -((-t0) // stride)
    return first, step, n, off0, (step * dil) // stride


def is_gather(row):
    return row.entry != 'wgrad'


def is_dgrad(row):
    return row.entry in ('dgrad', 'sums')


def gather_plan(row):
    """what hfwd_params / hconv_dgrad_impl and the kernel's prologue make of a row"""
    ho, wo = out_hw(row)
    if is_dgrad(row):
        m, kc = row.c, row.k
        cls = [fill_class_h(par, row.r, row.stride, row.pad, row.dil) for par in range(row.stride)]
        hc = [ceil_div(row.h - par, row.stride) for par in range(row.stride)]
        wc = [ceil_div(row.w - par, row.stride) for par in range(row.stride)]
        classes = [dict(taps=cls[a][2] * cls[b][2], cols=row.n * hc[a] * wc[b], image=hc[a] * wc[b], h=cls[a], w=cls[b]) for a in range(row.stride) for b in range(row.stride)]
    else:
        m, kc = row.k, row.c
        classes = [dict(taps=row.r * row.r, cols=row.n * ho * wo, image=ho * wo, h=None, w=None)]
    c8 = kc // 8
    for c in classes:
        c['chunks'] = c['taps'] * c8
        c['nk'] = ceil_div(c['chunks'], BK_CHUNKS)
    tiles_m = ceil_div(m, 128)
    m0 = (tiles_m - 1) * 128
    return dict(epi=epi_of(row), m=m, kc=kc, c8=c8, narrow=m <= 64, tiles_m=tiles_m, tiles_n=ceil_div(max(c['cols'] for c in classes), 128), classes=classes,
                npass_last=1 if (m <= 64 or m0 + 64 >= m) else 2, terms=row.r * row.r * kc + 4)


def hwgrad_plan(n, c, k, r, ho, wo):
    tiles = ceil_div(k, 128) * ceil_div(r * r * c, 128)
    ktot = n * ho * wo
    s = max(1, min(ceil_div(WGRAD_TARGET, tiles), ceil_div(ktot, 32 * 8)))
    kchunk = ceil_div(ceil_div(ktot, s), 32) * 32
    splits = ceil_div(ktot, kchunk)
    return splits, kchunk, ktot - (splits - 1) * kchunk


def wgrad_plan(row):
    ho, wo = out_hw(row)
    splits, kchunk, last = hwgrad_plan(row.n, row.c, row.k, row.r, ho, wo)
    return dict(splits=splits, kchunk=kchunk, last=last, tiles_m=ceil_div(row.k, 128), tiles_n=ceil_div(row.r * row.r * row.c, 128), ho=ho, wo=wo, ktot=row.n * ho * wo)


def reduce_loops(nsplit):
    """per slice sl of hwgrad_reduce_kernel: (four-slab trips, tail iterations)"""
    out = []
    for sl in range(8):
        sp, trips, tails = sl, 0, 0
        while sp + 24 < nsplit:
            trips, sp = trips + 1, sp + 32
        while sp < nsplit:
            tails, sp = tails + 1, sp + 8
        out.append((trips, tails))
    return out


def c_real(row):
    return 3 if 'creal3' in row.opts else 1 if 'creal1' in row.opts else row.c


def path(row):
    if row.entry == 'wgrad':
        p = wgrad_plan(row)
        return 's%d kc%d last%d m%d n%d' % (p['splits'], p['kchunk'], p['last'], p['tiles_m'], p['tiles_n'])
    p = gather_plan(row)
    s = 'E%d %s m%d n%d nk%s' % (p['epi'], 'narrow' if p['narrow'] else 'wide', p['tiles_m'], p['tiles_n'], ','.join(str(c['nk']) for c in p['classes']))
    return s + (' p%d' % p['npass_last'] if p['epi'] == 4 else '')


def geometry(row):
    return '%dx%ds%dp%dd%d' % (row.r, row.r, row.stride, row.pad, row.dil)


def features(row):
    """the paths and edges a row reaches, as names: REQUIRED lists what the table must reach between its rows"""
    o, f = set(row.opts), set()
    if row.entry == 'wgrad':
        p = wgrad_plan(row)
        key = (row.n, row.c, row.k, row.r, p['ho'], p['wo'])
        if key in WGRAD_PLANS:
            f.add('w:plan:%d' % p['splits'])
        loops = reduce_loops(p['splits'])
        both = sum(1 for t, u in loops if t and u)
        kind = 'tail' if not any(t for t, _ in loops) else 'either' if both == 0 else 'through1' if both == 1 else 'through8' if both == 8 else 'through'
        f.add('w:reduce:%s:acc%d' % (kind, int('acc' in o)))
        f.add('w:scale:%s' % ('small' if 'small' in o else 'one'))
        if p['wo'] == 1:
            f.add('w:Wo=1')
        if p['wo'] < 32:
            f.add('w:Wo<32')
        if p['ktot'] < 32:
            f.add('w:pixels<32')
        if p['last'] % 32:
            f.add('w:last_split_ragged')
        if (row.r * row.r * row.c) % 128:
            f.add('w:column_tile_ragged')                   # chunks past the last tap: b_ok
        if p['tiles_n'] > 1 and 128 % row.c:
            f.add('w:column_tile_ends_in_a_tap')
        if p['tiles_m'] > 1 and row.k % 128:
            f.add('w:second_row_tile_ragged')
        if p['splits'] < ceil_div(p['ktot'], 256):
            f.add('w:capped_by_target')
        if row.stride > 1:
            f.add('w:stride%d' % row.stride)
        if row.dil > 1 and row.pad > 0:
            f.add('w:dilated_padded')
        f |= {'w:' + v for v in o & {'xmask', 'creal3', 'creal1'}}
        return f
    p = gather_plan(row)
    e = p['epi']
    f.add('E%d:M%d' % (e, p['m']))
    if e == 0:
        f.add('E0:' + ('bias' if 'bias' in o else 'factor+accumulate'))
    if e == 1:
        f.add('E1:' + ('+'.join(sorted(o & {'mult', 'mask', 'acc'})) or 'plain'))
    if e == 4 and p['m'] in (72, 192, 200):
        f.add('E4:M%d:%s:%s' % (p['m'], '+'.join(sorted(o & {'res', 'relu'})) or 'none', 'all' if {'bias', 'mask', 'mult'} <= o else 'bare' if not o & {'bias', 'mask', 'mult'} else 'some'))
        f.add('E4:M%d:p%d' % (p['m'], p['npass_last']))
    big = max(p['classes'], key=lambda c: c['cols'])
    small = min(p['classes'], key=lambda c: c['cols'])
    if big['cols'] < 128:
        f.add('E%d:cols<128' % e)
    if big['cols'] == 128:
        f.add('E%d:cols=128' % e)
    if big['cols'] > 128 and big['cols'] % 128:
        f.add('E%d:second_tile_ragged' % e)
    if min(128, big['cols']) > 3 * big['image']:
        f.add('E%d:tile_spans_images' % e)
    if ceil_div(big['cols'], 128) > ceil_div(small['cols'], 128):
        f.add('class:block_past_its_columns')
    for c in p['classes']:
        nk = c['nk']
        f.add('nk%d' % nk if nk < 4 else 'nk_even' if nk % 2 == 0 else 'nk_odd')
        if nk == 1:
            f.add('nk1_full' if c['chunks'] == BK_CHUNKS else 'nk1_dead_chunks')
        if nk == 2:
            f.add('nk2:Kc%d' % p['kc'])
        if nk > 1 and c['chunks'] % BK_CHUNKS:
            f.add('last_step_dead_chunks')
        if c['taps'] > 1 and p['c8'] in (1, 3, 5):
            f.add('C8=%d' % p['c8'])
    if not is_dgrad(row):
        f.add('fwd:stride%d' % row.stride)
        if row.dil > 1:
            f.add('fwd:dil%d' % row.dil)
        if row.r == 7 and row.pad == 3:
            f.add('fwd:7x7p3')
        if row.r > 1 and row.pad == 0:
            f.add('fwd:no_padding')
        if row.h != row.w:
            f.add('fwd:H<W' if row.h < row.w else 'fwd:H>W')
    elif row.stride > 1:
        f.add('dgrad:%s:%s' % (geometry(row), '+'.join(sorted(o & {'acc', 'mask'})) or 'plain'))
        hs = [fill_class_h(par, row.r, row.stride, row.pad, row.dil) for par in range(row.stride)]
        if any(h[2] == 0 for h in hs):
            f.add('class:dead')
        if any(h[2] and h[3] < 0 for h in hs):
            f.add('class:negative_off0')
        if len({h[2] for h in hs}) > 1:
            f.add('class:unequal_taps')
        if any(h[2] > 1 and h[1] > 1 for h in hs):
            f.add('class:step>1')
        if row.stride > row.r:
            f.add('class:stride>R')
        if 'zpad' in o:
            f.add('dgrad:padding_channels')
    if row.entry == 'sums':
        f.add('E3:exact_zero_preactivation')
    return f


M_SWEEP = (8, 40, 64, 72, 128, 136, 200, 272)
DGRAD_GEOMETRIES = ('3x3s2p1d1', '1x1s2p0d1', '7x7s2p3d1', '3x3s2p2d2', '3x3s3p1d1', '5x5s3p2d1', '3x3s3p0d2', '1x1s4p0d1', '3x3s4p1d1', '7x7s4p3d1')
REQUIRED = (
    {'E%d:M%d' % (e, m) for e in range(5) for m in M_SWEEP}
    | {'E0:bias', 'E0:factor+accumulate', 'E1:plain', 'E1:mult', 'E1:acc', 'E1:mask'}
    | {'E4:M%d:%s:%s' % (m, v, w) for m in (72, 192, 200) for v in ('none', 'res', 'relu', 'relu+res') for w in ('bare', 'all')}
    | {'E4:M72:p2', 'E4:M200:p2', 'E4:M192:p1'}
    | {'E%d:%s' % (e, v) for e in range(5) for v in ('cols<128', 'cols=128', 'second_tile_ragged', 'tile_spans_images')}
    | {'nk0', 'nk1', 'nk2', 'nk3', 'nk_even', 'nk_odd', 'nk1_full', 'nk1_dead_chunks', 'nk2:Kc40', 'nk2:Kc64', 'last_step_dead_chunks', 'C8=1', 'C8=3', 'C8=5'}
    | {'fwd:stride1', 'fwd:stride2', 'fwd:stride3', 'fwd:stride4', 'fwd:dil2', 'fwd:dil4', 'fwd:7x7p3', 'fwd:no_padding', 'fwd:H<W', 'fwd:H>W'}
    | {'dgrad:%s:%s' % (g, v) for g in DGRAD_GEOMETRIES for v in ('plain', 'acc', 'mask', 'acc+mask')}
    | {'class:dead', 'class:negative_off0', 'class:unequal_taps', 'class:step>1', 'class:stride>R', 'class:block_past_its_columns', 'dgrad:padding_channels',
       'E3:exact_zero_preactivation'}
    | {'w:plan:%d' % v[0] for v in WGRAD_PLANS.values()}
    | {'w:reduce:%s:acc%d' % (k, a) for k in ('tail', 'either', 'through1', 'through8') for a in (0, 1)}
    | {'w:scale:one', 'w:scale:small', 'w:Wo=1', 'w:Wo<32', 'w:pixels<32', 'w:last_split_ragged', 'w:column_tile_ragged', 'w:column_tile_ends_in_a_tap', 'w:second_row_tile_ragged',
       'w:capped_by_target', 'w:stride2', 'w:stride3', 'w:dilated_padded', 'w:xmask', 'w:creal3', 'w:creal1'}
)

# the expected path of every row, written out (path(row) must give the same)
_S3 = ',1' * 8
_S4 = ',0' * 15
PATHS = {
    'm8_bias': 'E0 narrow m1 n1 nk5', 'm8_plain': 'E1 narrow m1 n1 nk5', 'm8_stats': 'E2 narrow m1 n1 nk5', 'm8_sums': 'E3 narrow m1 n1 nk5',
    'm8_infer': 'E4 narrow m1 n1 nk5 p1',
    'm40_bias': 'E0 narrow m1 n2 nk5', 'm40_plain': 'E1 narrow m1 n2 nk5', 'm40_mult': 'E1 narrow m1 n2 nk5', 'm40_stats': 'E2 narrow m1 n2 nk5',
    'm40_sums': 'E3 narrow m1 n2 nk5', 'm40_infer': 'E4 narrow m1 n2 nk5 p1',
    'm64_bias': 'E0 narrow m1 n1 nk5', 'm64_plain': 'E1 narrow m1 n1 nk5', 'm64_mult': 'E1 narrow m1 n1 nk5', 'm64_stats': 'E2 narrow m1 n1 nk5',
    'm64_sums': 'E3 narrow m1 n1 nk5', 'm64_infer': 'E4 narrow m1 n1 nk5 p1',
    'm72_bias': 'E0 wide m1 n2 nk5', 'm72_plain': 'E1 wide m1 n2 nk5', 'm72_stats': 'E2 wide m1 n2 nk5', 'm72_sums': 'E3 wide m1 n2 nk5',
    'm72_infer': 'E4 wide m1 n2 nk5 p2',
    'm128_bias': 'E0 wide m1 n1 nk5', 'm128_plain': 'E1 wide m1 n1 nk5', 'm128_stats': 'E2 wide m1 n1 nk5', 'm128_sums': 'E3 wide m1 n1 nk5',
    'm128_infer': 'E4 wide m1 n1 nk5 p2',
    'm136_bias': 'E0 wide m2 n2 nk5', 'm136_plain': 'E1 wide m2 n2 nk5', 'm136_mult': 'E1 wide m2 n2 nk5', 'm136_stats': 'E2 wide m2 n2 nk5',
    'm136_sums': 'E3 wide m2 n2 nk5', 'm136_infer': 'E4 wide m2 n2 nk5 p1',
    'm200_bias': 'E0 wide m2 n1 nk5', 'm200_plain': 'E1 wide m2 n1 nk5', 'm200_stats': 'E2 wide m2 n1 nk5', 'm200_sums': 'E3 wide m2 n1 nk5',
    'm200_infer': 'E4 wide m2 n1 nk5 p2',
    'm272_bias': 'E0 wide m3 n2 nk5', 'm272_plain': 'E1 wide m3 n2 nk5', 'm272_stats': 'E2 wide m3 n2 nk5', 'm272_sums': 'E3 wide m3 n2 nk5',
    'm272_infer': 'E4 wide m3 n2 nk5 p1',
    'i72_none': 'E4 wide m1 n2 nk3 p2', 'i72_res': 'E4 wide m1 n2 nk3 p2', 'i72_relu': 'E4 wide m1 n2 nk3 p2', 'i72_res_relu': 'E4 wide m1 n2 nk3 p2',
    'i72_all_none': 'E4 wide m1 n2 nk3 p2', 'i72_all_res': 'E4 wide m1 n2 nk3 p2', 'i72_all_relu': 'E4 wide m1 n2 nk3 p2', 'i72_all_res_relu': 'E4 wide m1 n2 nk3 p2',
    'i200_none': 'E4 wide m2 n2 nk3 p2', 'i200_res': 'E4 wide m2 n2 nk3 p2', 'i200_relu': 'E4 wide m2 n2 nk3 p2', 'i200_res_relu': 'E4 wide m2 n2 nk3 p2',
    'i200_all_none': 'E4 wide m2 n2 nk3 p2', 'i200_all_res': 'E4 wide m2 n2 nk3 p2', 'i200_all_relu': 'E4 wide m2 n2 nk3 p2', 'i200_all_res_relu': 'E4 wide m2 n2 nk3 p2',
    'i192_none': 'E4 wide m2 n2 nk3 p1', 'i192_res': 'E4 wide m2 n2 nk3 p1', 'i192_relu': 'E4 wide m2 n2 nk3 p1', 'i192_res_relu': 'E4 wide m2 n2 nk3 p1',
    'i192_all_none': 'E4 wide m2 n2 nk3 p1', 'i192_all_res': 'E4 wide m2 n2 nk3 p1', 'i192_all_relu': 'E4 wide m2 n2 nk3 p1', 'i192_all_res_relu': 'E4 wide m2 n2 nk3 p1',
    'cols128_bias': 'E0 wide m1 n1 nk3', 'cols128_plain': 'E1 wide m1 n1 nk3', 'cols128_stats': 'E2 wide m1 n1 nk3', 'cols128_sums': 'E3 wide m1 n1 nk3',
    'cols128_infer': 'E4 wide m1 n1 nk3 p2',
    'img3_bias': 'E0 wide m1 n2 nk3', 'img3_plain': 'E1 wide m1 n2 nk3', 'img3_stats': 'E2 wide m1 n2 nk3', 'img3_sums': 'E3 wide m1 n2 nk3',
    'img3_infer': 'E4 wide m1 n2 nk3 p2',
    'k_1x1_c8': 'E1 wide m1 n2 nk1', 'k_1x1_c32': 'E1 wide m1 n2 nk1', 'k_1x1_c40': 'E1 wide m1 n2 nk2', 'k_1x1_c64': 'E0 wide m1 n2 nk2',
    'k_3x3_c8': 'E1 wide m1 n2 nk3', 'k_1x1_c128': 'E1 wide m1 n2 nk4', 'k_3x3_c24': 'E0 wide m1 n2 nk7', 'k_3x3_c40': 'E1 wide m1 n2 nk12',
    'k_7x7_c8': 'E1 wide m1 n2 nk13', 'ki_1x1_c8': 'E4 wide m1 n2 nk1 p2', 'ki_3x3_c24': 'E4 wide m1 n2 nk7 p2',
    'kd_1x1_k8': 'E1 wide m1 n2 nk1', 'kd_1x1_k40': 'E1 wide m1 n2 nk2', 'kd_3x3_k8': 'E1 wide m1 n2 nk3', 'kd_3x3_k8_acc': 'E1 wide m1 n2 nk3',
    'kd_3x3_k8_mask': 'E1 wide m1 n2 nk3', 'kd_3x3_k8_both': 'E0 wide m1 n2 nk3', 'kd_3x3_k24': 'E1 wide m1 n2 nk7', 'kd_3x3_k40': 'E1 wide m1 n2 nk12',
    'g_s2': 'E1 narrow m1 n1 nk5', 'g_s2_stats': 'E2 narrow m1 n1 nk5', 'g_s3': 'E0 narrow m1 n1 nk5', 'g_s4': 'E1 narrow m1 n1 nk5',
    'g_s4_1x1': 'E1 narrow m1 n1 nk1', 'g_d2': 'E0 narrow m1 n3 nk5', 'g_d4': 'E1 narrow m1 n3 nk5', 'g_p0': 'E1 narrow m1 n2 nk5',
    'g_7x7': 'E0 narrow m1 n2 nk13', 'g_7x7s2': 'E4 narrow m1 n1 nk13 p1', 'g_s3_5x5': 'E2 narrow m1 n1 nk7', 'g_s2d2': 'E4 narrow m1 n1 nk5 p1',
    'd_3x3s2p1': 'E1 wide m1 n2 nk1,1,1,2', 'd_3x3s2p1_acc': 'E1 wide m1 n2 nk1,1,1,2', 'd_3x3s2p1_mask': 'E1 wide m1 n2 nk1,1,1,2',
    'd_3x3s2p1_both': 'E0 wide m1 n2 nk1,1,1,2', 'd_3x3s2p1_zpad': 'E1 narrow m1 n2 nk1,1,1,2', 'd_3x3s2p1_zpad_acc': 'E1 narrow m1 n2 nk1,1,1,2',
    'd_1x1s2': 'E1 narrow m1 n2 nk1,0,0,0', 'd_1x1s2_acc': 'E1 narrow m1 n2 nk1,0,0,0', 'd_1x1s2_mask': 'E1 narrow m1 n2 nk1,0,0,0',
    'd_1x1s2_both': 'E0 narrow m1 n2 nk1,0,0,0',
    'd_7x7s2p3': 'E1 narrow m1 n2 nk3,3,3,4', 'd_7x7s2p3_acc': 'E1 narrow m1 n2 nk3,3,3,4', 'd_7x7s2p3_mask': 'E1 narrow m1 n2 nk3,3,3,4',
    'd_7x7s2p3_both': 'E0 narrow m1 n2 nk3,3,3,4',
    'd_3x3s2p2d2': 'E1 wide m2 n2 nk3,0,0,0', 'd_3x3s2p2d2_acc': 'E1 wide m2 n2 nk3,0,0,0', 'd_3x3s2p2d2_mask': 'E1 wide m2 n2 nk3,0,0,0',
    'd_3x3s2p2d2_both': 'E0 wide m2 n2 nk3,0,0,0',
    'd_3x3s3p1': 'E1 narrow m1 n2 nk1' + _S3, 'd_3x3s3p1_acc': 'E1 narrow m1 n2 nk1' + _S3, 'd_3x3s3p1_mask': 'E1 narrow m1 n2 nk1' + _S3,
    'd_3x3s3p1_both': 'E0 narrow m1 n2 nk1' + _S3,
    'd_5x5s3p2': 'E1 wide m1 n2 nk1' + _S3, 'd_5x5s3p2_acc': 'E1 wide m1 n2 nk1' + _S3, 'd_5x5s3p2_mask': 'E1 wide m1 n2 nk1' + _S3,
    'd_5x5s3p2_both': 'E0 wide m1 n2 nk1' + _S3,
    'd_3x3s3p0d2': 'E1 wide m2 n2 nk1' + _S3, 'd_3x3s3p0d2_acc': 'E1 wide m2 n2 nk1' + _S3, 'd_3x3s3p0d2_mask': 'E1 wide m2 n2 nk1' + _S3,
    'd_3x3s3p0d2_both': 'E0 wide m2 n2 nk1' + _S3,
    'd_1x1s4': 'E1 wide m3 n2 nk1' + _S4, 'd_1x1s4_acc': 'E1 wide m3 n2 nk1' + _S4, 'd_1x1s4_mask': 'E1 wide m3 n2 nk1' + _S4, 'd_1x1s4_both': 'E0 wide m3 n2 nk1' + _S4,
    'd_3x3s4p1': 'E1 wide m1 n2 nk1,1,0,1,1,1,0,1,0,0,0,0,1,1,0,1', 'd_3x3s4p1_acc': 'E1 wide m1 n2 nk1,1,0,1,1,1,0,1,0,0,0,0,1,1,0,1',
    'd_3x3s4p1_mask': 'E1 wide m1 n2 nk1,1,0,1,1,1,0,1,0,0,0,0,1,1,0,1', 'd_3x3s4p1_both': 'E0 wide m1 n2 nk1,1,0,1,1,1,0,1,0,0,0,0,1,1,0,1',
    'd_7x7s4p3': 'E1 narrow m1 n2 nk1' + ',1' * 15, 'd_7x7s4p3_acc': 'E1 narrow m1 n2 nk1' + ',1' * 15, 'd_7x7s4p3_mask': 'E1 narrow m1 n2 nk1' + ',1' * 15,
    'd_7x7s4p3_both': 'E0 narrow m1 n2 nk1' + ',1' * 15,
    'w_tiny': 's1 kc32 last15 m1 n1', 'w_1x1': 's2 kc256 last256 m1 n1', 'w_c24': 's3 kc192 last160 m1 n2', 'w_7x7': 's5 kc224 last160 m1 n4',
    'w_s9': 's9 kc256 last208 m1 n2', 'w_s9_acc': 's9 kc256 last208 m1 n2', 'w_s32': 's32 kc256 last164 m1 n1', 'w_s32_acc': 's32 kc256 last164 m1 n1',
    'w_s33': 's33 kc256 last235 m1 n2', 'w_s33_acc': 's33 kc256 last235 m1 n2', 'w_s40': 's40 kc256 last16 m1 n1', 'w_s40_acc': 's40 kc256 last16 m1 n1',
    'w_s64': 's64 kc288 last288 m2 n3', 'w_s65': 's65 kc256 last256 m1 n1', 'w_wo1': 's1 kc128 last120 m1 n1', 'w_s2': 's1 kc224 last220 m1 n2',
    'w_s3': 's1 kc128 last112 m1 n2', 'w_d2': 's2 kc224 last166 m1 n2', 'w_xmask': 's4 kc224 last128 m1 n2', 'w_xmask_s2': 's3 kc192 last160 m1 n1',
    'w_creal3': 's3 kc192 last160 m1 n4', 'w_creal3_acc': 's3 kc192 last160 m1 n4', 'w_creal1': 's2 kc160 last112 m1 n4',
}
