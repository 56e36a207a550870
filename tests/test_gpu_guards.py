"""Memory discipline of every kernel entry of include/voxvae.h: an entry reads and writes only inside the tensors it was given, its
workspace is write-before-read (metrics_fwd alone and behind bce_fwd on one workspace) and its result does not depend on workspace_bytes beyond the minimum.

One row = one case of an existing oracle-parity test.  The row runs THAT test (so the plain result it is compared with has just been
held to the float64 oracle) while tests/_guarded.Recorder stands in for voxvae.lib's ptr() / call(), then replays every recorded launch
on guard-banded buffers (tests/_guarded.py): guards and inputs byte-identical afterwards, outputs bit-identical to the plain run, a
second run bit-identical, and for a workspace entry 0x00 / 0xFF pre-fills, an over-announced size and a one-byte-short size.  Kernel
forms are chosen by the parity test itself (monkeypatch.setenv on the VV_* overrides); the replay runs under the overrides it recorded.
The case tuples are checked against the parity tests' own parametrize lists by tests/test_guarded_host.py, which also compares
the entry names below with the header.

Entries of the header that launch a kernel and have no row here, and why:"""
import inspect

import pytest
import torch

import _guarded as G
import test_gpu_api as GA
import test_gpu_latent_ops as LO
import test_gpu_ops as O
import test_gpu_sampled as S
import test_gpu_train_ops as TO
import test_gpu_wgrad_exact as WX

LEFT_OUT = {
    'vv_pr_curve_accumulate': 'tests/test_gpu_prcurve.py already runs it between sentinels, accumulators and workspace included',
    'vv_voxel_points_count': 'tests/test_gpu_points.py runs count + emit between sentinels and against a host twin',
    'vv_voxel_points_emit': 'tests/test_gpu_points.py runs count + emit between sentinels and against a host twin',
    'vv_object_pose': 'tests/test_gpu_pose.py holds it bit for bit to the host twin compiled from the same code',
    'vv_adam_step_multi': 'its pointers sit in a device table, not in the argument list; tests/test_gpu_train_ops.py runs it between canaries',
    'vv_pack_skip_images': 'its pointers sit in host arrays, not in the argument list; held bit for bit to the single pack calls, which have rows',
}

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


class Row:
    def __init__(self, test, case, entries, tail):
        self.test, self.case, self.entries, self.tail = test, dict(case), set(entries), tail
        self.id = '%s-%s' % (test.__name__[5:], '-'.join(str(v) for v in self.case.values()))


ROWS = []


def row(test, names, values, entries, tail, **more):
    case = dict(zip(names.split(','), values))
    case.update(more)
    ROWS.append(Row(test, case, entries if isinstance(entries, (set, tuple, list)) else [entries], tail))


# ------------------------------------------------------------------------------------------ implicit GEMM (igemm.hip), three types
# rows M = B (side/2)^3 against the BM = 64 / 128 row tile; split-K where K = 64 cin is deep and M small
for dt in ('f32', 'bf16'):
    row(O.test_conv3d_k4s2, 'B,side,cin,cout', (1, 16, 64, 128), ['vv_pack_conv_k4', 'vv_conv3d_k4s2_fwd'], 'B = 1: M = 512, whole BM tiles, no split', dtname=dt)
    row(O.test_conv3d_k4s2, 'B,side,cin,cout', (3, 4, 128, 64), ['vv_pack_conv_k4', 'vv_conv3d_k4s2_fwd'], 'M = 24 rows: one partial BM tile', dtname=dt)
    row(O.test_conv3d_k4s2, 'B,side,cin,cout', (5, 2, 256, 512), ['vv_conv3d_k4s2_fwd'], 'M = 5 rows, K = 16384: split-K slabs in the workspace', dtname=dt)
    row(O.test_conv3d_k4s2, 'B,side,cin,cout', (37, 8, 64, 128), ['vv_conv3d_k4s2_fwd'], 'B >= 32: position-major rows, 37 of a BM tile', dtname=dt)
    row(O.test_convT3d_k4s2, 'B,side,cin,cout', (1, 8, 128, 64), ['vv_pack_convT_k4s2', 'vv_convT3d_k4s2_fwd'], 'B = 1: M = 512 per parity', dtname=dt)
    row(O.test_convT3d_k4s2, 'B,side,cin,cout', (3, 2, 512, 256), ['vv_pack_convT_k4s2', 'vv_convT3d_k4s2_fwd'], 'M = 24 rows per parity: a partial BM tile, split-K', dtname=dt)
    row(O.test_convT3d_k4s2, 'B,side,cin,cout', (33, 2, 64, 128), ['vv_convT3d_k4s2_fwd'], 'B >= 32: position-major rows, 33 of a BM tile', dtname=dt)
    row(O.test_dense, 'M,N,K', (4, 64, 64), ['vv_pack_dense', 'vv_dense_fwd'], 'M = 4 rows of a BM tile', dtname=dt)
    row(O.test_dense, 'M,N,K', (7, 128, 16), ['vv_dense_fwd'], 'M = 7, K = 16: less than one BK chunk', dtname=dt)
    row(O.test_dense, 'M,N,K', (2, 64, 8200), ['vv_dense_fwd'], 'K = 8200: split-K with a ragged last share', dtname=dt)
    row(O.test_dense, 'M,N,K', (130, 4096, 64), ['vv_dense_fwd'], 'M = 130 = two BM tiles + 2 rows', dtname=dt)
row(O.test_conv3d_k4s2_fp8, 'B,side,cin,cout,odt', (1, 16, 128, 64, 'f32'), ['vv_pack_conv_k4', 'vv_conv3d_k4s2_fwd_io'], 'B = 1, fp8 operands, f32 store')
row(O.test_conv3d_k4s2_fp8, 'B,side,cin,cout,odt', (37, 4, 256, 512, 'fp8'), ['vv_conv3d_k4s2_fwd_io'], 'B = 37 position-major rows, one-byte stores')
row(O.test_conv3d_k4s2_fp8, 'B,side,cin,cout,odt', (3, 8, 64, 128, 'bf16'), ['vv_conv3d_k4s2_fwd_io'], 'cin 64: tap-pair rows, M = 192 = BM + half a tile')
row(O.test_convT3d_k4s2_fp8, 'B,side,cin,cout,odt', (3, 8, 128, 64, 'bf16'), ['vv_pack_convT_k4s2', 'vv_convT3d_k4s2_fwd_io'], 'smallest fp8 case, bf16 store')
row(O.test_convT3d_k4s2_fp8, 'B,side,cin,cout,odt', (33, 2, 512, 256, 'fp8'), ['vv_convT3d_k4s2_fwd_io'], 'B = 33 position-major rows, split-K')
row(O.test_dense_and_convert_fp8, '', (), ['vv_dense_fwd', 'vv_convert', 'vv_pack_dense'], 'M = 37 rows of a BM tile, fp8 operands and fp8 store; vv_convert at 4096 elements')

# ------------------------------------------------------------------------ skip / position-major / whole-sample kernels (bf16)
# skip_direct.hip keeps four samples per workgroup (SD_ATILE = [4 s][4][4][4] rows)
row(O.test_conv3d_k4s2_skip, 'B,cin,cout,act', (5, 64, 64, 1), ['vv_pack_conv_k4_skip', 'vv_conv3d_k4s2_skip_fwd'], 'B = 5: last quad holds one sample')
row(O.test_conv3d_k4s2_skip, 'B,cin,cout,act', (33, 64, 128, 1), ['vv_conv3d_k4s2_skip_fwd'], 'B = 33: nine quads, last holds one sample')
row(O.test_convT3d_k4s2_skip, 'B,cin,cout,act', (3, 64, 128, 1), ['vv_pack_convT_k4s2_skip', 'vv_convT3d_k4s2_skip_fwd'], 'B = 3: one quad, one sample short')
row(O.test_convT3d_k4s2_skip, 'B,cin,cout,act', (33, 128, 128, 1), ['vv_convT3d_k4s2_skip_fwd'], 'B = 33: nine quads, last holds one sample')
# posgemm.hip: PG_BM = 256 batch rows per tile, PG_BN = 128 channels; the split count follows the batch
row(O.test_conv3d_k4s2_pos, 'B,cin,cout,act', (5, 64, 64, 1), ['vv_conv3d_k4s2_pos_fwd'], 'B = 5 of PG_BM = 256 rows, cout 64 of PG_BN = 128')
row(O.test_conv3d_k4s2_pos, 'B,cin,cout,act', (37, 256, 512, 1), ['vv_conv3d_k4s2_pos_fwd'], 'B = 37 of PG_BM rows, deep K: several shares per position')
row(O.test_conv3d_k4s2_pos, 'B,cin,cout,act', (300, 64, 128, 1), ['vv_conv3d_k4s2_pos_fwd'], 'B = 300 = PG_BM + 44: a second, partial sample tile')
row(O.test_conv3d_k4s2_pos, 'B,cin,cout,act', (256, 128, 136, 1), ['vv_conv3d_k4s2_pos_fwd'], 'cout 136 = PG_BN + 8: a channel-tail tile')
row(O.test_convT3d_k4s2_pos, 'B,cin,cout,act', (3, 64, 64, 1), ['vv_convT3d_k4s2_pos_fwd'], 'B = 3 of PG_BM = 256 rows')
row(O.test_convT3d_k4s2_pos, 'B,cin,cout,act', (40, 512, 256, 1), ['vv_convT3d_k4s2_pos_fwd'], 'B = 40 of PG_BM rows, deep K')
row(O.test_convT3d_k4s2_pos, 'B,cin,cout,act', (290, 64, 128, 1), ['vv_convT3d_k4s2_pos_fwd'], 'B = 290 = PG_BM + 34')
row(O.test_convT3d_k4s2_pos, 'B,cin,cout,act', (256, 128, 72, 1), ['vv_convT3d_k4s2_pos_fwd'], 'cout 72: a channel tail inside one PG_BN tile')
# convt_whole.hip: one workgroup per (sample, parity split); every MFMA form x every parity split the parity test runs
for shape in (16, 32, 4):
    for ps in (0, 1, 2, 4, 8):
        row(O.test_convT3d_k4s2_whole, 'B,act,ps,shape', (3, 1, ps, shape), ['vv_convT3d_k4s2_whole_fwd'], 'B = 3, 8 / ps parities per workgroup; the last sample ends the buffer')
    row(O.test_convT3d_k4s2_whole, 'B,act,ps,shape', (33, 2, 0, shape), ['vv_convT3d_k4s2_whole_fwd'], 'B = 33: the automatic parity split at an odd batch')
row(O.test_convT3d_whole_stats_form, 'B', (3,), ['vv_convT3d_k4s2_whole_stats_fwd', 'vv_bn_finalize_stats', 'vv_bn_train_stats'], 'B = 3 blocks of column sums; 12288 rows in the statistics sweep')

# ---------------------------------------------------------------------------------------- direct E2 / D4 kernels and fp8 twins
# conv_direct.hip: 4x8x8 output boxes, side 16 -> two boxes per sample; convt_direct.hip: 4x4x8 cell blocks
for shape in (16, 32, 8):
    row(O.test_conv3d_k4s2_direct, 'B,side,act,shape', (1, 16, 3, shape), ['vv_conv3d_k4s2_direct_fwd'], 'B = 1: two boxes, the last box ends the buffer')
    row(O.test_conv3d_k4s2_direct, 'B,side,act,shape', (3, 16, 0, shape), ['vv_conv3d_k4s2_direct_fwd'], 'B = 3: six boxes, odd against the two workgroups per CU of shape 8')
for variant in ('8', '4', '2'):
    row(O.test_convT3d_k4s2_direct, 'B,side,variant', (1, 16, variant), ['vv_pack_convT_k4s2_frag', 'vv_convT3d_k4s2_direct_fwd'], 'B = 1: halo tiles at the grid faces')
    row(O.test_convT3d_k4s2_direct, 'B,side,variant', (3, 8, variant), ['vv_convT3d_k4s2_direct_fwd'], 'B = 3, side 8: four blocks per sample, every block touches a face')
row(O.test_conv3d_direct_fp8_output, '', (), ['vv_conv3d_k4s2_direct_fwd_io'], 'B = 2, e4m3 store')
row(O.test_conv3d_direct_fp8, 'B,side,act,odt', (1, 16, 1, 'bf16'), ['vv_conv3d_k4s2_direct_fp8_fwd'], 'B = 1, bf16 store')
row(O.test_conv3d_direct_fp8, 'B,side,act,odt', (3, 16, 0, 'fp8'), ['vv_conv3d_k4s2_direct_fp8_fwd'], 'B = 3, e4m3 store: six boxes')
row(O.test_convT3d_direct_fp8, 'B,side,act', (1, 8, 1), ['vv_pack_convT_k4s2_frag_fp8', 'vv_convT3d_k4s2_direct_fp8_fwd'], 'B = 1, both stores')
row(O.test_convT3d_direct_fp8, 'B,side,act', (3, 8, 0), ['vv_convT3d_k4s2_direct_fp8_fwd'], 'B = 3, both stores')

# --------------------------------------------------------------------------------------------------------- first / last layer
for dt in ('f32', 'bf16'):
    row(O.test_conv3d_first, 'B,D', (1, 16), ['vv_conv3d_first_fwd'], 'B = 1, gather form', dtname=dt)
    row(O.test_conv3d_first, 'B,D', (3, 8), ['vv_conv3d_first_fwd'], 'B = 3 at D = 8: 192 output rows, gather form', dtname=dt)
    row(O.test_conv3d_first, 'B,D', (7, 32), ['vv_conv3d_first_fwd'], 'B = 7: plane form (bf16), a ragged last workgroup', dtname=dt)
row(O.test_conv3d_first_gather_form_at_plane_sizes, 'B,D', (1, 32), ['vv_conv3d_first_fwd'], 'B = 1, VV_FIRSTCONV_GATHER at a plane-form grid')
row(O.test_conv3d_first_gather_form_at_plane_sizes, 'B,D', (7, 32), ['vv_conv3d_first_fwd'], 'B = 7, VV_FIRSTCONV_GATHER: a ragged last workgroup')
row(O.test_conv3d_first_fp8_output, 'B,D', (2, 32), ['vv_conv3d_first_fwd_io'], 'plane form, e4m3 store')
for out in ('bf16', 'fp8'):     # chained and VV_FIRSTCONV_NOCHAIN plane forms; 65 samples leave a ragged last workgroup of chains
    row(O.test_conv3d_first_chained_equals_plane_form, 'B,D,act', (65, 32, 1), ['vv_conv3d_first_fwd_io'], 'B = 65: chains of two, ragged last workgroup', out=out)
    row(O.test_conv3d_first_chained_equals_plane_form, 'B,D,act', (9, 64, 1), ['vv_conv3d_first_fwd_io'], 'B = 9 at 64^3: ragged last workgroup', out=out)
# final_bce.hip: box form 4^3 cells + halo per workgroup (FM_ROWS), sweep forms 8x8 tiles (FL_ROWS = 100 halo rows)
FINAL = ['vv_convT3d_final_bce_fwd', 'vv_convT3d_final_bce_metrics_fwd', 'vv_shape_metrics']
for dt, B, side, form in (('f32', 3, 4, 'box'), ('f32', 1, 8, 'box'), ('bf16', 3, 4, 'box'), ('bf16', 1, 8, 'box'), ('bf16', 3, 8, 'sweep'), ('bf16', 1, 32, 'sweep'),
                          ('bf16', 3, 8, 'sweepp'), ('bf16', 2, 16, 'sweepp')):
    row(O.test_convT3d_final_bce, 'B,side,form', (B, side, form), FINAL, 'B = %d: %s' % (B, 'one box per sample' if side == 4 else 'the last tile ends the buffer'), dtname=dt)
row(O.test_convT3d_final_bce_fp8_input, 'B,side', (3, 8), ['vv_convT3d_final_bce_fwd'], 'B = 3, e4m3 input, one 8x8 tile per plane')
row(O.test_convT3d_final_bce_fp8_input, 'B,side', (1, 32), ['vv_convT3d_final_bce_fwd'], 'B = 1, e4m3 input')
for dt in ('f32', 'bf16'):      # final_mean.hip: the K samples of an object split over workgroups (at most 8 partial grids)
    row(S.test_convT3d_final_mean, 'B,K,side', (1, 32, 8), ['vv_convT3d_final_mean_fwd'], 'one object, K = 32: partial grids in the workspace', dtname=dt)
    row(S.test_convT3d_final_mean, 'B,K,side', (5, 3, 4), ['vv_convT3d_final_mean_fwd'], 'B = 5, K = 3: odd against every split', dtname=dt)
row(S.test_sample_latents, 'B,K,Lz', (1, 32, 16), ['vv_sample_latents'], 'one object')
row(S.test_sample_latents, 'B,K,Lz', (3, 5, 64), ['vv_sample_latents'], '960 elements: a partial last block')

# ------------------------------------------------------------------------------------------------------------------ latent tail
# latent_tail.hip: LT_BM = 128 batch rows x LT_BN = 64 columns, K staged LT_KS = 256 at a time
row(O.test_latent_tail, 'B,K5,Lz,lin,n1,variational', (5, 1024, 32, 512, 2048, True), ['vv_latent_tail_fwd'], 'B = 5 of LT_BM = 128 rows')
row(O.test_latent_tail, 'B,K5,Lz,lin,n1,variational', (19, 8200, 64, 96, 80, True), ['vv_latent_tail_fwd'], 'K5 = 8200: a ragged LT_KS slice; n1 = 80 = LT_BN + 16')
row(O.test_latent_tail, 'B,K5,Lz,lin,n1,variational', (37, 4096, 64, 64, 4096, False), ['vv_latent_tail_fwd'], 'B = 37, autoencoder form (no eps, no kl)')
row(O.test_conv_pos_latent_tail_fused, 'B,cin,cout,Lz,variational', (5, 64, 256, 64, True), ['vv_conv_pos_latent_tail_fwd', 'vv_conv3d_k4s2_pos_fwd', 'vv_latent_tail_fwd'], 'B = 5 of PG_BM / LT_BM rows')
row(O.test_conv_pos_latent_tail_fused, 'B,cin,cout,Lz,variational', (37, 64, 256, 32, True), ['vv_conv_pos_latent_tail_fwd'], 'B = 37 of PG_BM / LT_BM rows, E = 64')
row(O.test_reparam_kl, '', (), ['vv_reparam_kl_fwd'], 'B = 5 / 3 / 2 at L = 64 / 16 / 100: L = 100 is no multiple of the wave')

# ----------------------------------------------------------------------------------------------------- latent.hip / small.hip
row(LO.test_nearest_category, 'B,Lz,C,kind,maskkind', (1, 16, 129, 'clustered', 'none'), ['vv_nearest_category'], 'B = 1, C = 129 = two waves of classes + 1')
row(LO.test_nearest_category, 'B,Lz,C,kind,maskkind', (300, 16, 40, 'random', 'half'), ['vv_nearest_category'], 'B = 300 rows with a mask')
for act in ('null', 'bf16'):
    row(LO.test_latent_mask_fill, 'B,Lz,C,act', (1, 16, 40, act), ['vv_latent_mask_fill'], '16 elements: part of one block')
    row(LO.test_latent_mask_fill, 'B,Lz,C,act', (3, 100, 1, act), ['vv_latent_mask_fill'], '300 elements: a block + 44')
    row(LO.test_latent_correct, 'B,Lz,C,act', (1, 16, 40, act), ['vv_latent_correct'], '16 elements: part of one block')
    row(LO.test_latent_correct, 'B,Lz,C,act', (65, 16, 200, act), ['vv_latent_correct'], '1040 elements: four blocks + 16')
row(LO.test_category_accuracy, 'B,C', (1, 40), ['vv_category_accuracy'], 'B = 1')
row(LO.test_category_accuracy, 'B,C', (65, 200), ['vv_category_accuracy'], 'B = 65: a wave + 1')
row(LO.test_binary_loss_and_counts, 'B,V,k', (1, 1, 0), ['vv_binary_loss', 'vv_voxel_precision_recall'], 'one voxel')
row(LO.test_binary_loss_and_counts, 'B,V,k', (5, 255, 1), ['vv_binary_loss', 'vv_voxel_precision_recall'], 'V = 255: one short of a block, rows at odd 4-byte offsets')
row(LO.test_binary_loss_and_counts, 'B,V,k', (256, 257, 2), ['vv_binary_loss', 'vv_voxel_precision_recall'], 'V = 257: a block + 1')
row(LO.test_kl_loss, 'B,Lz', (1, 16), ['vv_kl_loss'], 'B = 1, L = 16')
row(LO.test_kl_loss, 'B,Lz', (37, 100), ['vv_kl_loss'], 'L = 100: no multiple of the wave')
row(LO.test_sampling, 'n', (1,), ['vv_sampling'], 'one element')
row(LO.test_sampling, 'n', (257,), ['vv_sampling'], 'a block + 1')
row(LO.test_regulizer_loss, 'B,Lz,cdim', (1, 16, 0), ['vv_regulizer_loss'], 'B = 1')
row(LO.test_regulizer_loss, 'B,Lz,cdim', (37, 16, 5), ['vv_regulizer_loss'], 'B = 37 pairs rows with classes')
row(LO.test_regulizer_loss, 'B,Lz,cdim', (257, 64, 5), ['vv_regulizer_loss'], 'B = 257: a block of rows + 1')
row(LO.test_shape_metrics, 'B', (1,), ['vv_shape_metrics'], 'B = 1')
row(LO.test_shape_metrics, 'B', (65,), ['vv_shape_metrics'], 'B = 65: a wave + 1')
row(LO.test_max_over_positions, 'B,npos,C,negative', (1, 1, 7, False), ['vv_max_over_positions'], 'seven channels')
row(LO.test_max_over_positions, 'B,npos,C,negative', (37, 8, 128, False), ['vv_max_over_positions'], '4736 outputs: a partial last block')
row(TO.test_sigmoid_f32_against_float64, 'in_place', (False,), ['vv_sigmoid_f32'], 'out of place')
row(TO.test_sigmoid_f32_against_float64, 'in_place', (True,), ['vv_sigmoid_f32'], 'in place: x is y')
# a whole model against the CPU oracle: every launch of the engine, on the engine's own grow-only workspace sizes, at B = 5
row(GA.test_encoder_final_pool_max, 'dtype,D', ('f32', 16), ['vv_pack_conv_k4s1_full', 'vv_max_over_positions', 'vv_fold_bn'], 'B = 5 through every layer of the 16^3 model, final_pool = max')
row(GA.test_encoder_final_pool_max, 'dtype,D', ('bf16', 32), ['vv_pack_conv_k4s1_full', 'vv_max_over_positions', 'vv_fold_bn'], 'B = 5 through every layer of the 32^3 model, bf16 kernel forms')
row(GA.test_bit_packed_device_data_path, '', (), ['vv_pack_bits', 'vv_unpack_bits_gather'], '5 x 4096 voxels packed, 3 rows gathered out of order')

# ----------------------------------------------------------------------------------------------------------------- training ops
# bn.hip statistics / wgrad.hip kernels cut the rows into blocks (BR = 32 / 64 rows a chunk) whose partials land in the workspace
for dt in ('f32', 'bf16'):
    row(O.test_batchnorm_train_ops, 'rows,C', (777, 128), ['vv_bn_train_stats', 'vv_bn_act_fwd', 'vv_bn_act_bwd'], 'rows = 777: odd against every row block', dtname=dt)
    row(O.test_batchnorm_train_ops, 'rows,C', (5, 256), ['vv_bn_train_stats', 'vv_bn_act_fwd', 'vv_bn_act_bwd'], 'rows = 5: fewer rows than a block', dtname=dt)
    row(O.test_colsum, 'rows,C', (3, 64), ['vv_colsum'], 'three rows', dtname=dt)
    row(O.test_colsum, 'rows,C', (1000, 40), ['vv_colsum'], 'C = 40: a partial column block', dtname=dt)
for adt, gdt in (('f32', 'f32'), ('bf16', 'bf16'), ('bf16', 'f32')):     # dense: rows 300 / 1000 ragged against BR, m = 160 against BM = 128; conv: cin 1 / 64 / 128; VV_WGRAD_F32
    row(O.test_wgrad_kernels, 'adt,gdt', (adt, gdt), ['vv_wgrad_dense', 'vv_wgrad_conv_k4s2'], 'rows 300 / 1000, m = 160, n = 96; B = 3 / 5 / 2 conv gathers')
# wgrad_phase.hip: NS samples per box, an odd batch leaves the last box half empty
row(O.test_wgrad_conv_phase_form, 'B,side,cin,cout', (1, 32, 64, 128), ['vv_wgrad_conv_k4s2'], 'B = 1, phase and reduction-GEMM forms')
row(O.test_wgrad_conv_phase_form, 'B,side,cin,cout', (5, 16, 64, 128), ['vv_wgrad_conv_k4s2'], 'B = 5: the last box half empty')
row(O.test_wgrad_conv_phase_form, 'B,side,cin,cout', (17, 8, 64, 128), ['vv_wgrad_conv_k4s2'], 'B = 17: NS = 16 samples per box + 1')
# kernel forms only the exact tests reach (tests/test_gpu_wgrad_exact.py): a pitched A on either kernel, the full-tile single-channel bf16 kernel, side 2
for dt in ('f32', 'bf16'):
    row(WX.test_wgrad_dense_exact, 'rows,m,n,lda,adt,gdt', (300, 160, 96, 192, dt, dt), ['vv_wgrad_dense'], 'lda = 192 against m = 160: the last row ends 32 elements before the buffer does')
    row(WX.test_wgrad_conv_exact, 'B,side,cin,cout,sdt,gdt', (5, 2, 64, 64, dt, dt), ['vv_wgrad_conv_k4s2'], 'side 2: five rows, half the taps of every row are padding')
row(WX.test_wgrad_conv_exact, 'B,side,cin,cout,sdt,gdt', (2, 8, 1, 128, 'f32', 'bf16'), ['vv_wgrad_conv_k4s2'], 'one source channel, cout 128: shifted 16-byte loads at both ends of a grid row')
row(TO.test_adam_step_against_float64, 'n,t,layer', (1, 1, False), ['vv_adam_step'], 'one element')
row(TO.test_adam_step_against_float64, 'n,t,layer', (257, 2, False), ['vv_adam_step'], 'a block + 1')
row(TO.test_adam_step_against_float64, 'n,t,layer', (16385, 7, True), ['vv_adam_step'], 'a 16384-element chunk + 1')
for use_mask in (False, True):
    row(TO.test_reparam_kl_bwd_against_float64_autograd, 'B,Lz,use_mask', (1, 32, use_mask), ['vv_reparam_kl_bwd'], 'B = 1')
    row(TO.test_reparam_kl_bwd_against_float64_autograd, 'B,Lz,use_mask', (5, 100, use_mask), ['vv_reparam_kl_bwd'], 'L = 100: no multiple of the wave')
row(TO.test_bce_bwd_at_real_sizes_against_float64_autograd, 'B,D', (1, 32), ['vv_bce_bwd'], 'B = 1')
row(TO.test_bce_bwd_at_real_sizes_against_float64_autograd, 'B,D', (5, 32), ['vv_bce_bwd'], 'B = 5')
row(TO.test_meanpool_panel_pack_layout_and_adjoint, 'S,cin,cout', (1, 512, 128), ['vv_pack_conv_k4s1_meanpool', 'vv_unpack_meanpool_grad'], 'S = 1')
row(TO.test_meanpool_panel_pack_layout_and_adjoint, 'S,cin,cout', (2, 24, 40), ['vv_pack_conv_k4s1_meanpool', 'vv_unpack_meanpool_grad'], 'ragged channels 24 / 40')
row(TO.test_convT_dense_panel_pack_layout_and_adjoint, 'S,cin,cout', (1, 8, 512), ['vv_pack_convT_k4s1_dense', 'vv_unpack_convT_dense_grad'], 'S = 1')
row(TO.test_convT_dense_panel_pack_layout_and_adjoint, 'S,cin,cout', (4, 3, 7), ['vv_pack_convT_k4s1_dense', 'vv_unpack_convT_dense_grad'], 'ragged channels 3 / 7')
row(TO.test_transpose_f32_exact, 'rows,cols', (1, 1), ['vv_transpose_f32'], 'one element')
row(TO.test_transpose_f32_exact, 'rows,cols', (33, 65), ['vv_transpose_f32'], '32 x 32 tiles + 1 in both directions')
row(TO.test_fold_bn_against_float64, 'channels,repeat,with_bias', (37, 1, True), ['vv_fold_bn'], '37 channels')
row(TO.test_fold_bn_against_float64, 'channels,repeat,with_bias', (3, 64, False), ['vv_fold_bn'], 'three channels tiled 64 times, no bias')


@pytest.fixture(scope='module')
def L():
    from voxvae import lib
    lib.load()
    assert torch.cuda.is_available()
    return lib


@pytest.mark.parametrize('r', ROWS, ids=[r.id for r in ROWS])
def test_memory_discipline(L, r, monkeypatch):
    for v in L.HOOK_VARS:
        monkeypatch.delenv(v, raising=False)
    rec = G.Recorder(L).install(monkeypatch)
    kwargs, params = dict(r.case), inspect.signature(r.test).parameters
    if 'L' in params:
        kwargs['L'] = L
    if 'monkeypatch' in params:
        kwargs['monkeypatch'] = monkeypatch
    r.test(**kwargs)                                   # the parity test itself: its plain outputs are held to the oracle here
    torch.cuda.synchronize()
    units = rec.units(skip=LEFT_OUT)
    names = {u[-1].name for u in units}
    assert r.entries <= names, 'the parity test did not launch %s' % sorted(r.entries - names)
    print('\n[%s] %d launches replayed: %s' % (r.id, len(units), ' '.join(sorted({u[-1].name for u in units}))))
    for u in units:
        G.guard_unit(L, u, DEV)


# ------------------------------------------------------------------------- the checker's own controls, on the device
def _device_arena():
    a = G.Arena(DEV)
    x = a.input(torch.arange(3 * 700, dtype=torch.float32, device=DEV).view(3, 700), 'x')
    y = a.output((3, 8, 5), torch.bfloat16, 'y')
    ws = a.workspace(1000, 0x00, 'ws')
    a.commit()
    return a, x, y, ws


def test_device_arena_untouched_passes_and_flips_are_reported():
    a, x, y, ws = _device_arena()
    assert x.address % 512 == 0 and y.address % 512 == 0 and ws.address % 512 == 0
    y.tensor.zero_()
    ws.payload.fill_(7)
    torch.cuda.synchronize()
    a.check()
    for b, off, side, rel in ((x, x.off - 1, 'leading guard', -1), (y, y.off + y.nbytes, 'trailing guard', y.nbytes), (x, x.off + 11, 'input payload', 11),
                              (ws, ws.off + ws.nbytes + ws.trail - 1, 'trailing guard', ws.nbytes + ws.trail - 1)):
        a, x, y, ws = _device_arena()
        a.base[off] ^= 1                               # torch indexing into the test's own allocation
        torch.cuda.synchronize()
        with pytest.raises(AssertionError) as e:
            a.check()
        assert "buffer '%s'" % b.name in str(e.value) and side in str(e.value) and 'first at payload offset %d,' % rel in str(e.value), str(e.value)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16] + ([G.torch.float8_e4m3fn] if hasattr(torch, 'float8_e4m3fn') else []))
def test_device_one_element_past_an_input_poisons_a_reduction(dtype):
    a = G.Arena(DEV)
    b = a.input(torch.ones(4, 33, device=DEV).to(dtype), 'x')
    a.commit()
    assert float(b.raw().float().sum()) == 4 * 33
    assert bool(torch.isnan(b.raw(elements_past_end=1).float().sum()))
