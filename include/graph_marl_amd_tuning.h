/* Tuning and diagnostic switches of libgraphmarl_amd (not part of the reference-facing interface:
 * a binding of the reference's call sites never needs them; tools/ and the A/B benches do). Every
 * switch selects among kernel forms with the same arithmetic contract; the defaults are the
 * measured-best forms. */
#pragma once
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Tuning knob: tile configuration of gm_gemm_f32 (-1 = per-shape default; 0 = 128x128x32;
 * 1 = 128x256x16; 2 = 256x128x16 (LSTM: 256x128x16); 3 = 128x128x16; 4 = 128x128x16 at 4
 * blocks/CU); of gm_gemm_x3 (-1/0 = 128x128x16; 1 = 128x256x16 (LSTM: 128x128x32);
 * 2 = 128x128x32 (LSTM: 256x128x16)); 8..14 the LDS-DMA tiles of gm_gemm_x3's dense / readout
 * sources (8 = 256x256, 9 = 128x256 3 stages, 10 = 128x256, 12 = 128x128 2 blocks/CU, 13 = 128x128
 * of 64x64 waves, 14 = 128x256 of 64x128 waves). Process-wide. */
/* Weight-gradient kernel of gm_gemm_x3_wgrad (same arithmetic, diagnostics / A-B timing):
 * -1 (default) or 1 = transposed LDS reads (ds_read_b64_tr_b16) with 128 x 128 tiles, 2 = the same
 * with 128 x 256 tiles, 3 = 128 x 128 tiles on v_mfma_f32_16x16x32_f16, 0 = the dword-load
 * register-transpose form (tools/wgrad_bench.py). + 8: the same form with the blocks in dispatch order
 * (default: the tiles of a k chunk grouped on one XCD). */
int gm_gemm_set_wgrad(int32_t form);
int gm_gemm_set_tile(int32_t tile);
/* MFMA shape of the LDS-DMA split-f16 kernel (gm_gemm_x3's dense / readout tiles, gm_gemm_x3_head):
 * 2 (default) = v_mfma_f32_16x16x32_f16 everywhere, 1 = 16x16x32 except gm_gemm_x3_head (32x32x16),
 * 0 = v_mfma_f32_32x32x16_f16 everywhere. Same tiles and operand images; the summation order inside
 * an MFMA differs (fp32-order results either way). */
int gm_gemm_set_mfma(int32_t shape);
/* Input-gradient kernel of gm_gemm_x3_dgrad (same arithmetic and epilogue contract; A-B timing):
 * -1 (default) = per-shape choice, 0 = register-staged 128 x 128 tile (k_gemm3), 1 = LDS-DMA
 * 128 x 128 tile (4 waves, 2 blocks/CU), 2 = LDS-DMA 128 x 256 tile (8 waves). Process-wide. */
int gm_gemm_set_dgrad(int32_t form);
/* Form of gm_mp_iterate / gm_mp_iterate_bwd (same arithmetic, bit for bit; A-B timing, tools/stateless_bench.py):
 * -1 (default) = per-shape choice (LDS-resident where the graph fits, for iters >= 2 and for iters = 1 on small
 * graphs), 0 = always
 * the chained per-round launches, 1 = the LDS-resident launch wherever the shape allows it (iters = 1 too).
 * Process-wide. */
int gm_mp_iterate_set_form(int32_t form);
/* Arithmetic form the GEMM kernels were compiled with, e.g. "x3=lo12 diag=0": x3=lo12 = split-f16
 * with the A operand's low piece scaled by 2^12 in every kernel (the only form since round 5);
 * diag = 0 for the product build, 30 for the k-step stamp build (tools/stamp_bench.py). */
const char* gm_gemm_form(void);
/* Diagnostic: the kernel the most recent call on this thread of a dispatching entry point launched ("" before
 * the first such call). NetMon: gm_netmon_readout[_ld], gm_netmon_readout_bwd[_sym], gm_mp_aggregate[_rows|_bwd],
 * gm_mp_iterate[_bwd] ("k_mp_iterate<fwd|bwd>" or the last chained kernel), gm_lstm_cell_bwd and gm_qhead_bwd
 * report a string literal such as "k_readout_bwd_cs<2>/S=8". GEMMs:
 * gm_gemm_f32 (gm_linear_f32), gm_gemm_x3, gm_gemm_x3_dgrad, gm_gemm_x3_head, gm_encoder_x3 and
 * gm_gemm_x3_wgrad[2] report the instantiation with its template parameters, e.g.
 * "k_gemm<2,2,2,2,BK16,DENSE,BIAS,occ2>", "k_gemm3<4,1,1,4,BK16,AGGREGATE,LSTM,occ2>" (wave grid WGM x WGN,
 * 32x32 tiles per wave TM x TN, k tile, A source, epilogue, blocks per CU),
 * "k_gemm3g<4,2,1,4,S3,DENSE,BIAS,occ1,AX1,MF1>" (.., stages, .., AX 0 plain / 1 publishes max|A| / 2 scaled A,
 * MF 0 32x32x16 / 1 16x16x32 MFMA), "k_gemm3_kmajor", "k_wgrad_tr<128,0>" (tile width, MFMA form) with "/xcd"
 * appended when the k chunks are grouped per XCD. One thread-local state for both families, one host store
 * per call, nothing on the device; the tests of the dispatch thresholds read it
 * (tests/test_netmon_paths_gpu.py, tests/test_gemm_paths_gpu.py), the product never does. */
const char* gm_last_kernel(void);
/* The same for gm_lnlstm_fwd / gm_lnlstm_pointwise alone ("k_lnlstm_pw<1|2|4|8>", "" before the first call): a
 * slot of its own, so that gm_last_kernel reads after those two calls what it read before they named a kernel
 * (the recorded launch lists of the sequence-batched update depend on it). tests/test_encoder_cells_paths_gpu.py. */
const char* gm_last_lnlstm_pw(void);
/* The i-th kernel name the GEMM entry points of this build can report through gm_last_kernel, NULL past the
 * end: exactly the instantiations the two GEMM launchers were compiled for, plus the weight-gradient forms.
 * Filled when the library loads; needs no GPU. tests/test_gemm_paths_gpu.py requires a case for every name. */
const char* gm_gemm_kernel_name(int32_t i);

#ifdef __cplusplus
}
#endif
