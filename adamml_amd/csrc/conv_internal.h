// Internal launchers of libadamml_hip: every function that one csrc/*.hip file defines and another one calls is declared HERE and nowhere
// else, and both sides include this header: a signature is written once, so a caller cannot hold a stale copy of it (with C++ linkage
// that compiled, linked and failed only as an unresolved symbol when the library was loaded).  Default arguments live here only.
// Declarations only: no .hip file keeps a prototype of a function it does not define (tests/test_host_cpu.py checks both).  The C ABI is
// include/adamml_hip.h; the error plumbing every file uses is in common.h.
//
// `d` is the descriptor conv_launch (conv_gemm.hip) dispatches on -- for a data gradient the flipped one (dgrad_desc) -- unless noted.
#pragma once
#include "common.h"
#include "../../include/adamml_hip.h"

// ---- conv_wgrad.hip: the split reduce behind every kernel that writes one partial per workgroup
// dw[perm(i)] (+)= sum_{s<nsplit} ws[g][s][i] for the `groups` outputs of n indices each; taps > 1: ws is [co][tap][cin], dw [co][cin][tap];
// store: overwrite instead of accumulate.  No launch check: the callers below and conv_launch's product form add their own
void launch_wgrad_reduce(const float* ws, float* dw, size_t n, int nsplit, int taps, int cin, int store, int groups, hipStream_t stream);
// dw[perm(i)] += sum_{s<nsplit} ws[s*n + i]
int adamml_launch_split_reduce(const float* ws, float* dw, size_t n, int nsplit, hipStream_t stream, int taps = 1, int cin = 1);
// per-group form: ws [groups][nsplit][n] -> out [groups][n], OVERWRITTEN (the products of the algebraic BatchNorm backward)
int adamml_launch_split_reduce_grouped(const float* ws, float* out, size_t n, int nsplit, int groups, int cin, hipStream_t stream);

// ---- conv3x3_c64.hip: 3x3 / 64 -> 64 convs of ResNet layer 1 (forward and data gradient; weight gradient with one partial per workgroup)
bool adamml_conv3x3_c64_supported(const adamml_conv_desc_t* d);
int adamml_conv3x3_c64_launch(const adamml_conv_desc_t* d, const void* x, const void* w_packed, const float* in_scale,
                              const float* in_shift, void* y, double* stats, const void* bn_z, const float* bn_vec, int bn_act,
                              hipStream_t stream);
// the residual form of the data gradient (adamml_conv_bwd_data_res without a second BatchNorm operand); d->accumulate: dx holds the
// identity-path gradient
bool adamml_conv3x3_c64_res_supported(const adamml_conv_desc_t* d);
int adamml_conv3x3_c64_res_launch(const adamml_conv_desc_t* d, const void* dz, const void* w_dgrad_packed, void* dx, const void* res_out,
                                  const uint8_t* res_mask, int res_act, const void* z_a, const float* vec_a, double* sums_a, hipStream_t stream);
bool adamml_conv3x3_c64_wgrad_supported(const adamml_conv_desc_t* d, int cin_true);
int adamml_conv3x3_c64_wgrad_blocks(const adamml_conv_desc_t* d, int* tpb_out);
int adamml_conv3x3_c64_wgrad_launch(const adamml_conv_desc_t* d, const void* dz, const void* x, const float* in_scale,
                                    const float* in_shift, float* ws, hipStream_t stream);

// ---- conv1x1_narrow.hip: narrow 1x1 convs of the MobileNetV2s (barrier-free streaming kernels)
bool adamml_conv1x1_narrow_fwd_supported(const adamml_conv_desc_t* d);
int adamml_conv1x1_narrow_fwd_launch(const adamml_conv_desc_t* d, const void* x, const void* w_packed, const float* in_scale, const float* in_shift,
                                     void* y, double* stats, hipStream_t stream);
bool adamml_conv1x1_narrow_wgrad_supported(const adamml_conv_desc_t* d, int cin_true);
int adamml_conv1x1_narrow_wgrad_launch(const adamml_conv_desc_t* d, const void* dz, const void* x, const float* in_scale, const float* in_shift,
                                       float* ws, int max_blocks_per_group, int* nblk_out, hipStream_t stream);
// (d: the FORWARD descriptor, as adamml_conv_bwd_data_dual receives it)
bool adamml_conv1x1_narrow_dual_supported(const adamml_conv_desc_t* d);
int adamml_conv1x1_narrow_dual_launch(const adamml_conv_desc_t* d, const void* g, const void* z, const float* aff, void* dz_side,
                                      const void* w_dgrad_packed, void* dx, int accumulate, const void* z_in, const float* bn_vec, int act,
                                      double* sums, hipStream_t stream);
bool adamml_conv1x1_narrow_dgrad_epi_supported(const adamml_conv_desc_t* d);
int adamml_conv1x1_narrow_dgrad_epi_launch(const adamml_conv_desc_t* d, const void* dz, const void* w_packed, void* dx, const void* z_in,
                                           const float* bn_vec, int act, double* sums, hipStream_t stream);

// ---- conv1x1_wide.hip: expanding 1x1 convs of ResNet layers 3-4 (activation-stationary streaming kernel)
bool adamml_conv1x1_wide_expand_supported(const adamml_conv_desc_t* d);
int adamml_conv1x1_wide_expand_launch(const adamml_conv_desc_t* d, const void* x, const void* w_packed, const float* in_scale, const float* in_shift,
                                      void* y, double* stats, hipStream_t stream);

// ---- conv1x1_fadd_stream.hip: conv + BatchNorm + add (+ temporal pool) at the layer-2 shape, wave-slice streaming form
int adamml_conv1x1_fadd_stream_supported(const adamml_conv_desc_t* d);
int adamml_conv1x1_fadd_stream_launch(const adamml_conv_desc_t* d, const void* x, const void* w_packed, const float* in_scale, const float* in_shift,
                                      const float* bn_vec, const void* idn, const float* id_scale, const float* id_shift, int id_gstride, int act,
                                      void* out, uint8_t* mask_out, hipStream_t stream);
int adamml_conv1x1_fadd_tpool_stream_supported(const adamml_conv_desc_t* d, int frames);
int adamml_conv1x1_fadd_tpool_stream_launch(const adamml_conv_desc_t* d, const void* x, const void* w_packed, const float* in_scale, const float* in_shift,
                                            const float* bn_vec, const void* idn, const float* id_scale, const float* id_shift, int id_gstride, int act,
                                            int frames, void* pooled, uint16_t* code, hipStream_t stream);

// ---- conv1x1_fadd_next.hip: the streaming forms for layer 1 (64 -> 256), with the next block's conv1 or the temporal pool behind them
bool adamml_conv1x1_fadd_next_supported(const adamml_conv_desc_t* d, int next_cout);
int adamml_conv1x1_fadd_next_launch(const adamml_conv_desc_t* d, const void* x, const void* w_packed, const float* in_scale, const float* in_shift,
                                    const float* bn_vec, const void* idn, const float* id_scale, const float* id_shift, int id_gstride, int act,
                                    void* out, uint8_t* mask_out, const void* w1_packed, void* y1, double* stats1, hipStream_t stream);
bool adamml_conv1x1_fadd_tpool_supported(const adamml_conv_desc_t* d, int frames);
int adamml_conv1x1_fadd_tpool_launch(const adamml_conv_desc_t* d, const void* x, const void* w_packed, const float* in_scale, const float* in_shift,
                                     const float* bn_vec, const void* idn, const float* id_scale, const float* id_shift, int id_gstride, int act,
                                     int frames, void* pooled, uint16_t* code, hipStream_t stream);

// ---- conv1x1_stream.hip: the algebraic data gradient at the layer-1 shape (d: the FORWARD descriptor)
bool adamml_alg_stream_supported(int Cout, int Cin);
int adamml_alg_stream_launch(const adamml_conv_desc_t* d, const void* g, const void* a, const float* a_scale, const float* a_shift,
                             const void* w_alg, const float* epi_add, void* dx, int accumulate, const void* z_in, const float* bn_vec,
                             int act, double* sums, hipStream_t stream);

// ---- res_prod_stream.hip: residual data gradients, barrier-free streaming forms (d: the FORWARD descriptor)
int adamml_res_stream_supported(const adamml_conv_desc_t* d);
int adamml_res_stream_launch(const adamml_conv_desc_t* d, const void* dz, const void* w_dgrad_packed, void* dx, const uint8_t* res_mask, double* sums_a,
                             const void* z_b, const float* vec_b, double* sums_b, hipStream_t stream);
int adamml_res_prod_stream_supported(const adamml_conv_desc_t* d, int a_channels);
size_t adamml_res_prod_stream_workspace(const adamml_conv_desc_t* d);
int adamml_res_prod_stream_launch(const adamml_conv_desc_t* d, const void* dz, const void* w_dgrad_packed, void* dx, const uint8_t* res_mask,
                                  double* sums_a, const void* a, const float* a_scale, const float* a_shift, int a_act, int a_gstride,
                                  float* prod, void* workspace, size_t workspace_bytes, hipStream_t stream);
