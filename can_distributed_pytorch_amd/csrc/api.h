// C ABI of the HIP kernel translation units (one launcher per kernel family).
// Return value: 0 ok, >0 hipError_t, <0 argument/shape error.
// dt selects the 16-bit element type of activations / weight packs: 0 = bf16, 1 = fp16.
#pragma once
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int can_conv_igemm_batched(const void* x, const void* w, const float* bias, void* y, int nb, long long xbs,
                           long long wbs, long long ybs, int N, int H, int W, int Cin, int Cout, int ksize, int dil,
                           int epi, int tile_cfg, int dt, void* stream);
int can_conv_igemm(const void* x, const void* w, const float* bias, const void* mask, void* y, int N, int H, int W,
                   int Cin, int Cout, int ksize, int dil, int epi, int first, int tile_cfg, int dt, void* stream,
                   float* bpart, int bpart_cap, int* bpart_rows, const void* mbits_in, void* mbits_out, int wv);

int can_wgrad_plan(int M, int Cin, int Cout, int ksize, int first, int target_blocks, int* S_out, int* mslice_out,
                   int* cfg_out, int dil, int W);
// the weight-gradient launchers plan their launch themselves (wgrad_plan.h); ws_floats: the size of ws
int can_conv_wgrad(const void* dy, const void* x, float* ws, long long ws_floats, float* dw, float* db, int N, int H,
                   int W, int Cin, int Cout, int ksize, int dil, int first, float beta, float scale,
                   const float* dscale, int dt, void* stream, const float* bext, int bext_rows);
// stream events from one ring: record on a stream (returns the slot, < 0 error), wait for a slot, or both
int can_event_record(void* stream);
int can_event_wait(void* stream, int slot);
int can_stream_wait(void* dst, void* src);

// [R][C] fp32 rows -> <= rows_out rows (fixed-order block sums); returns the rows written (< 0: error)
int can_bias_rows_reduce(const float* in, float* out, int R, int C, int rows_out, void* stream);
int can_conv_wgrad_1x1_batched(const void* dy, const void* x, float* ws, long long ws_floats, float* dw, int M, int W,
                               int Cin, int Cout, int nb, long long dy_bs, long long x_bs, long long dw_bs, int ncu,
                               float beta, float scale, const float* dscale, int dt, void* stream);

// conv + bias + ReLU with the 2x2/s2 max-pool fused into the epilogue (y full resolution, yp pooled)
// codes: max-pool codes uint32 [N][H/2][W/2][Cout/8] (optional), y optional (nullptr: not written)
int can_conv_pool_fwd(const void* x, const void* w, const float* bias, void* y, void* yp, void* codes, int N, int H,
                      int W, int Cin, int Cout, int ksize, int dil, int tile_cfg, int dt, void* stream, int wv);
int can_conv_pool_tp(int Cin, int Cout, int ksize, int tile_cfg);

// conv1_2 with conv1_1's output recomputed from the NHWC4 image (never stored)

// conv1_2's data gradient with conv1_1's weight gradient fused (slabs [S][36][64] + [S][64]; returns S or < 0)
int can_conv_ws64_dgrad_w1g(const void* dy, const void* w, const void* mask, const void* img, void* y, float* w1slab,
                            float* w1bslab, int slab_cap, int N, int H, int W, int dt, void* stream,
                            const void* mbits);
int can_wgrad_reduce_first(const float* ws, const float* wsb, float* dw, float* db, int S, float beta, float scale,
                           const float* dscale, void* stream);

// elementwise.hip
int can_maxpool_fwd(const void* x, void* y, void* codes, int N, int H, int W, int C, int dt, void* stream);
int can_maxpool_bwd_codes(const void* codes, const void* dy, void* dx, int N, int H, int W, int C, int dt,
                          void* stream);
int can_maxpool_bwd_relu(const void* x, const void* dy, void* dx, int N, int H, int W, int C, int dt, void* stream);
int can_head_fwd(const void* y, const float* w, const float* b, float* et, int P, int dt, void* stream, int pitch,
                 int wv);
int can_head_train(const void* y, const float* w, const float* b, const float* gt, float* et, void* dy, float* part,
                   int nblk, float* dw, float* db, float* loss, int P, float gscale, float beta, const float* lscale,
                   float* nonfinite, int dt, void* stream, int pitch, int wv, const float* wt);
// wt (null: none): the per-pixel loss weight, P floats indexed and padded like gt (head_train_kernel<DT, true>)
// masked counts and GAME 0..3 per sample, two launches, fixed order: out [n][6] doubles = (E, G, GAME_0..GAME_3)
int can_count_metrics(const float* et, const float* gt, long long gt_stride, const float* m, long long m_stride, int n,
                      int h, int w, double* part, double* out, void* stream);
int can_sgd_momentum(float* p, float* buf, const float* g, size_t n, float lr, float momentum, float gscale,
                     int first, float* flags, const float* lr_dev, void* stream, const float* gmul);
int can_grad_nonfinite(const float* g, size_t n, float* flags, void* stream);
int can_split_x3(const float* src, void* dst, long long M, int C, int stride, int mode, int pattern, void* stream);
int can_scale_update(const float* flags, float* scaler, int interval, float growth, float backoff, float max_scale,
                     void* stream);
int can_pack_multi(const long long* desc, int layers, int max_tiles, int dt, void* stream);
int can_adam(float* p, float* m, float* v, const float* g, size_t n, float lr, double beta1, double beta2, float eps,
             float wd, int decoupled, float gscale, int step, int* t_dev, float* flags, const float* lr_dev,
             void* stream, const float* gmul);
// the fused optimizer step; eoff != 0: the EMA of the parameters is updated in the same launch (eoff: the EMA arena's
// offset from the masters in floats, ema_t: device count of applied updates)
int can_opt_pack(const long long* desc, int rows, int max_tiles, int opt, long long goff, long long boff,
                 long long voff, float lr, float momentum, double beta1, double beta2, float eps, float wd,
                 int decoupled, float gscale, int* t_dev, float* flags, const float* lr_dev, int dt, void* stream,
                 const float* gmul, long long eoff, double ema_decay, int ema_warmup, int* ema_t);
// the stand-alone EMA update and the master <-> EMA swap launch
int can_ema(float* e, const float* p, size_t n, double decay, int warmup, int step, int* t_dev, float* flags,
            void* stream);
int can_swap_pack(const long long* desc, int rows, int max_tiles, long long eoff, int dt, void* stream);
// gradient-norm pass over the fp32 arena (two launches, fixed order) and the accumulation window's loss tick
int can_grad_norm_chunk();
int can_grad_norm(const float* g, const long long* tab, int np, long long max_count, double* part, float* gn,
                  float gscale, float max_norm, float* flag, void* stream);
int can_accum_tick(float* flags, float* acc, int fold, int close, void* stream);
int can_img_to_nhwc4(const float* img, void* out, int N, int H, int W, int dt, void* stream);

// context.hip
int can_ctx_reduce(int mode, const void* in0, const void* sdir, const void* dc, float* rowacc, float* cells, int N,
                   int h, int w, int C, int dt, void* stream, int wv);
int can_ctx_expand(const void* fv, const float* T, void* cs, int N, int h, int w, int C, int dt, void* stream);
int can_ctx_fuse(const void* fv, const void* ws, const float* T, void* cat, int N, int h, int w, int C, int dt,
                 void* stream);
int can_ctx_bwd_e1(const void* dcat, const void* ws, const float* T, void* dz, void* sdir, int N, int h, int w, int C,
                   int dt, void* stream);
// 1: matrix-core kernel, 0: tiled kernel, < 0: refused (the choice can_ctx_gemm makes; host only)
int can_ctx_gemm_form(int N, int C);
int can_ctx_gemm(int mode, const float* x, const float* y, const float* const* w, float* out, float* const* gw, int N,
                 int C, float beta, float scale, const float* dscale, void* stream);
// linearised context module (conv_igemm.hip EPI_CTXF / EPI_CTXB + context.hip ctx_bwd_lin)
int can_conv_ctx(int fwd, const void* x, const void* w, const float* tab0, const float* tab1, const void* fv, void* cat,
                 void* y, int N, int H, int W, int C, int dt, void* stream, int wv);
int can_ctx_bwd_lin(const void* dcat, const void* wts, const float* U, void* dg, float* rowacc, int N, int h, int w,
                    int C, int dt, void* stream, int wv);
int can_ctx_cells(const float* rowacc, float* cells, int N, int h, int C, void* stream, const float* rowacc2,
                  float* cells2);
int can_ctx_w2_scatter(const float* tmp, float* const* dst, int C, float beta, void* stream);
int can_ctx_bwd_final(const void* dcat, const void* dc, const float* dave, const void* fv, void* dfv, int N, int h,
                      int w, int C, int dt, void* stream);

// density.hip
int can_density_map(const float* pts, int n, int H, int W, float* sigma_ws, float* out, int max_r, void* stream,
                    float fixed_sigma);
// ground truth of crop windows from head records (c, r, sigma, R): exact area sums, no atomics, table order.  The check
// reads host memory only and launches nothing; can_gt_from_heads runs it first and returns its code.
int can_gt_from_heads_check(const float* heads_host, long long n_heads, const long long* ranges_host,
                            const long long* desc_host, int n, int CH, int CW, int ds);
int can_gt_from_heads(const float* heads, const long long* ranges, const long long* desc, const float* heads_host,
                      long long n_heads, const long long* ranges_host, const long long* desc_host, int n, float* gt,
                      int CH, int CW, int ds, void* stream);

// preprocess.hip
int can_preprocess_image(const void* img, int H0, int W0, int C, int flip, void* out, int Ho, int Wo, int dt,
                         void* stream);
// resize batch, one launch: packed uint8 images, desc [n][8] int64 (device) = {image byte offset, H0, W0, C, flip, 0, 0,
// 0}, every image resampled whole to Ho x Wo (Wo even, x4 16-byte aligned).  Images only: a pack carries its ground
// truth at 1/ds resolution already, so dens and gt must be null; -2 for a non-null one, before any launch.
int can_preprocess_batch(const void* imgs, const float* dens, const long long* desc, int n, void* x4, float* gt,
                         int Ho, int Wo, int ds, int dt, void* stream);
// random-crop batch, one launch, no resize: desc [n][8] int64 = {image byte offset, H0, W0, C, flip, y0, x0, 1} on the
// device and (desc_host) on the host, where every window is checked against its image and img_bytes before the launch
int can_preprocess_crop(const void* imgs, long long img_bytes, const long long* desc, const long long* desc_host,
                        int n, void* x4, int CH, int CW, int ds, int dt, void* stream);
// random-scale crop batch, one launch of can_preprocess_batch's kernel: as can_preprocess_crop with slot 7 of a
// descriptor = (sh << 32) | sw, the extent of the window at (y0, x0) that is resampled (cv2 INTER_LINEAR, taps clamped
// inside the window) to CH x CW; refuses
// what can_preprocess_crop refuses, a window that is empty or leaves its image, and sh, sw beyond [CH/4, 4 CH], [CW/4, 4 CW]
int can_preprocess_crop_scaled(const void* imgs, long long img_bytes, const long long* desc,
                               const long long* desc_host, int n, void* x4, int CH, int CW, int ds, int dt,
                               void* stream);
// either crop launch (scaled == 0: can_preprocess_crop, else can_preprocess_crop_scaled) with photometric jitter: photo,
// float [n][260] on the device (16-byte aligned) and photo_host on the host, one row per output sample of 256 tone-table
// entries on the 0..255 scale, the gray flag (0 / 1) and three zeros.  Every source byte goes through its sample's table
// (and the luma mix where the flag is 1) before the resample.  Refuses what the plain entry refuses, a null or misaligned
// photo, an entry that is not finite or leaves [0, 255] and any other flag, before the launch
int can_preprocess_crop_photo(const void* imgs, long long img_bytes, const long long* desc, const long long* desc_host,
                              int n, void* x4, int CH, int CW, int ds, int dt, void* stream, const float* photo,
                              const float* photo_host, int scaled);
// ROI weight plane of a packed batch of any kind whose images are 4-channel (the mask is the alpha byte): out
// [n][2][CH/ds][CW/ds] fp32, plane 0 a copy of gt [n][CH/ds][CW/ds], plane 1 the weights (exact area means of alpha / 255
// over each cell's source rectangle; 0 in the padding cells of an unscaled crop).  The check reads host memory only and
// launches nothing: -31 an image that is not 4-channel, -32 a sample size that is no multiple of ds, -33 a window that
// is empty or leaves its image (-2: any other bad argument); can_roi_weights runs it first and returns its code.
int can_roi_weights_check(const long long* desc_host, int n, long long img_bytes, int CH, int CW, int ds);
int can_roi_weights(const void* imgs, long long img_bytes, const long long* desc, const long long* desc_host, int n,
                    const float* gt, float* out, int CH, int CW, int ds, void* stream);
// synthetic batch: full-res densities [n][H][W] + coarse noise [n][3][H/16][W/16] -> x4 NHWC4, gt [n][H/8][W/8]
int can_synth_render(const float* dens, const float* noise, float* dmax, void* x4, float* gt, int n, int H, int W,
                     int dt, void* stream);
int can_preprocess_density(const float* d, int H0, int W0, int flip, float* out, int Ho, int Wo, float mult,
                           void* stream);

// CUs of the current device, asked once (0: no device), and a 4-KiB page of zeros on it (nullptr: allocation failed):
// one of each for every kernel family (defined in conv_igemm.hip)
int can_device_cus();
const void* can_zero_page();

// views of the launch plan (conv_plan.h plan_conv) under the process's dispatch config
int can_conv_plan(int H, int W, int Cin, int Cout, int ksize, int dil, int epi);
int can_splitk_plan(int N, int H, int W, int Cin, int Cout, int ksize, int dil, int epi);
int can_splitk_dirty();
int can_splitk_slots_used();

#ifdef __cplusplus
}
#endif
