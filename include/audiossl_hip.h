/* audiossl_hip.h - C ABI of libaudiossl_hip.so (AMD MI355X / gfx950 only).
 *
 * The reference (Sreyan88/audio-ssl) has no native layer: its hot path is ATen ops called from
 * Python.  This header is therefore the boundary a reference maintainer would bind with ctypes
 * (see INTEGRATION.md); each entry point names the reference code it replaces (file:line under
 * the reference root).
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error (AUDIOSSL_E*); nothing throws;
 *   - all pointers are DEVICE pointers owned by the caller (no allocation, no ownership transfer),
 *     16-byte aligned, contiguous unless a leading dimension is given;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); launches are asynchronous;
 *   - `dtype` selects the storage/MFMA type of activations: 0 = fp32 (exact f32 MFMA, validation /
 *     high-precision path), 1 = bf16 (fp32 accumulate; master weights, statistics and losses stay fp32);
 *   - activations of the conv encoder are channels-last [N][T][F][64] (time, mel, channel), i.e. the
 *     reference's x.permute(0,3,2,1) (src/encoder/audiontt.py:76,83,90,95), so its feature index d*64+c
 *     is contiguous;
 *   - gradient outputs named d* are ACCUMULATED (+=) into caller-zeroed buffers;
 *   - `gdtype` (backward kernels of BatchNorm / pooling): storage type of the INCOMING gradient tensor - 0 = fp32 even
 *     when `dtype` is bf16 (it is a GEMM output, so fp32 is free, and BatchNorm's backward cancels most of it); the
 *     outgoing gradient is stored in `dtype` because it is only ever an MFMA operand;
 *   - `adtype` / `ydtype`: storage type of a BatchNorm INPUT (projector pre-activations, conv outputs) - 0 = fp32 also on
 *     the bf16 path: pre-normalisation values can have |mean| >> std, which 8 significand bits cannot carry.
 */
#ifndef AUDIOSSL_HIP_H
#define AUDIOSSL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AUDIOSSL_OK 0
#define AUDIOSSL_EINVAL (-1)   /* bad shape / null pointer / unsupported configuration */
#define AUDIOSSL_ELAUNCH (-2)  /* HIP reported an error at launch */
#define AUDIOSSL_EALIGN (-3)   /* pointer / leading dimension not 16-byte aligned */

/* ---- K1 front end: src/utils/utils.py:20-28 (MelSpectrogramLibrosa.__call__), :43-49 (log) ------------
 * wave [B][L] f32 -> out [B][n_mels][T] f32, T = 1 + L/hop, centre reflect pad, periodic Hann `win`[1024],
 * `tw` = exp(-2 pi i k/1024) as [1024][2], `melw` [n_mels][taps] = packed non-zero run of each filterbank
 * row starting at bin mel_start[m]; out = mel(|X|^2 + eps_pow), or log(. + eps_log) when apply_log.  n_fft must be 1024. */
int audiossl_logmel_fwd(const float* wave, float* out, int B, int L, int T, int n_fft, int hop, int n_mels, int taps,
                        const float* win, const float* tw, const float* melw, const int* mel_start, float eps_pow,
                        float eps_log, int apply_log, void* stream);
/* Ragged batch (whole-clip embeddings): wave [B][Lmax] holds lens[b] samples at the head of row b (the rest
 * of the row is never read), out [B][n_mels][Tmax].  Frames t < 1 + lens[b]/hop are those of clip b alone, the centre reflection
 * taken at the clip's own end; frames after them are exact zeros (a store each, no FFT).  lens: int32 [B] on the device; lens_host
 * (required): the caller's HOST copy, checked before the launch - EINVAL unless 1120 <= lens_host[b] <= Lmax for every b and
 * Tmax >= 1 + max(lens)/hop.  hop and Lmax even, wave 8-byte aligned (EALIGN); tables as for logmel_fwd. */
int audiossl_logmel_ragged_fwd(const float* wave, const int* lens, const int* lens_host, float* out, int B, int Lmax, int Tmax,
                               int n_fft, int hop, int n_mels, int taps, const float* win, const float* tw, const float* melw,
                               const int* mel_start, float eps_pow, float eps_log, int apply_log, void* stream);

/* ---- K1b Kaldi fbank front end of the MAST loader: extras/mast_new/mast/dataloader.py:129-130 (kaldi.fbank, htk_compat,
 * hanning, dither 0), :132-142 (cut / zero-pad to target_length), :187-202 (FrequencyMasking, TimeMasking, (x - mean) / (2 std)),
 * :105-127 (two-file mix) --------------------------------------------------------------------------------------------------
 * wave [B][Lmax] f32, lens [B] (NULL: every clip is Lmax long) -> out [B][1][n_mels][T_target] f32, or [B][T_target][n_mels]
 * when time_major.  Clip b has 1 + (len_b - win_len)/shift frames (0 when len_b < win_len, no centre padding); each frame
 * loses its mean, is pre-emphasised (y[i] = x[i] - preemph x[i-1], x[-1] = x[0]), multiplied by `win`[win_len] (symmetric
 * Hann), zero-padded to n_fft = 512 (256 < win_len <= 512) and transformed with `tw` = exp(-2 pi i k/512) as [512][2]; power bins
 * 0..255 go through `melw` [n_mels][taps] = packed non-zero run of each filterbank row starting at bin mel_start[m]
 * (taps <= 29, n_mels <= 128) into log(max(., eps_log)).  Frames past the clip's last up to T_target are 0, frames past T_target are
 * dropped; cells with mel row in [f0,f1) or frame in [t0,t1) of `bands` [B][4] = {f0,f1,t0,t1} (NULL: no masks) become 0; unless
 * skip_norm every cell, padding and masked ones included, becomes (v - mean) / (2 std).
 * bands_host (optional) is the caller's HOST copy of `bands`: when given it is checked against [0,n_mels] / [0,T_target] before the
 * launch.  partner [B] (-1: none) and lam [B] (both or neither): samples are lam w[b] + (1 - lam) w[partner[b]], the partner
 * zero-padded or cut to len_b.  clip_mean [B] (optional scratch, only with partner): a first launch fills it with the whole-clip
 * means and the mix uses w - mean (dataloader.py:108-109; without a mix the per-frame mean removal cancels it exactly). */
int audiossl_fbank_fwd(const float* wave, const int* lens, const int* partner, const float* lam, float* clip_mean,
                       const int* bands, const int* bands_host, float* out, int B, int Lmax, int win_len, int shift, int n_fft, int n_mels,
                       int taps, int T_target, const float* win, const float* tw, const float* melw, const int* mel_start,
                       float preemph, float eps_log, float mean, float std, int skip_norm, int time_major, void* stream);

/* ---- K2 RunningNorm: src/augmentations/augmentations.py:215-282 ----------------------------------------
 * clip_moments: mom[c] = {sum x, sum x^2} (fp64) of clip c over n = F*T elements.
 * runnorm_scan: sequential recurrence over the batch; state_i = {n_seen, max_update}, state_f = {mu, s2};
 *               writes the (mean, std) each clip is normalised with. */
int audiossl_clip_moments(const float* x, double* mom, int B, int n, void* stream);
int audiossl_runnorm_scan(const double* mom, int B, int n_elem, long long* state_i, float* state_f, float* mu_out,
                          float* sd_out, void* stream);
/* bank[(slot0 + c) % R][:] = (x[c] - mu[c]) / sd[c]; the ring is also the MixupBYOLA memory bank. */
int audiossl_aug_normalize(const float* x, const float* mu, const float* sd, float* bank, long slot0, int R, int B, int n,
                           void* stream);
/* ---- K3+K4 MixupBYOLA + RandomResizeCrop: augmentations.py:8-12, 97-111 and :40-55 ---------------------
 * ip [B][2][8] = {self_slot, partner_slot | -1, i, j, h, w, do_rrc, 0}; fp [B][2][2] = {coef_self, coef_partner}.
 * out1/out2 [B][F][T] f32 = the two views. */
int audiossl_aug_views(const float* bank, int R, const int* ip, const float* fp, float* out1, float* out2, int B, int F,
                       int T, int canvas_h, int canvas_w, int log_mix, void* stream);
/* ---- host planner (CPU function, HOST pointers, no stream): the reference's per-clip random draws, batched ---------
 * Continues numpy's legacy global MT19937 (np_key[624], *np_pos) and python `random`'s MT19937 (py_key, *py_pos) in
 * the reference's draw order (augmentations.py:32-37, 99-102; specaugment.py:80-88) and fills the aug_views /
 * mask_fill tables.  *n_entries = entries appended so far to MixupBYOLA's virtual FIFO (updated).  lens/unit/starts
 * (optional): the random window crop of src/utils/utils.py:166-182, drawn per clip ahead of that clip's views. */
int audiossl_aug_plan_host(uint32_t* np_key, int* np_pos, uint32_t* py_key, int* py_pos, int B, int F, int T,
                           long long clips_seen, long long* n_entries, int R, int n_memory, int use_mix, double ratio,
                           int use_rrc, double fs_lo, double fs_hi, double ts_lo, double ts_hi, int canvas_h,
                           int canvas_w, int use_spec, int spec_F, int spec_T, int spec_nf, int spec_nt, const int* lens,
                           int unit, int* starts, int* ip, float* fp, int* masks);

/* ---- K5 SpecAugment band masks: extras/delores-s/specaugment.py:68-122 ---------------------------------
 * tab [n_img][max_masks][4] = {axis (0 time, 1 freq, -1 stop), start, end, 0}; in place on x [n_img][F][T]. */
/* ---- f2 audio ingest: the resampling of `librosa.core.load(path, sr=16000)` (src/dataset/upstream_dataset.py:55; librosa 0.8.1
 * -> resampy 0.2.2, filter kaiser_best).  y[c][t] = sum_i (win[off_l[t] + i s] + eta_l[t] delta[...]) x[c][n[t] - i]
 *                                              + sum_k (win[off_r[t] + k s] + eta_r[t] delta[...]) x[c][n[t] + 1 + k],  s = index_step,
 * wings cut at the clip ends and the table end, products in fp64 added into an fp32 running sum in resampy's order.  The
 * position tables come from the host (src/dataset/ingest.py), which keeps resampy's float64 time register. */
int audiossl_resample_sinc(const float* x, float* y, int clips, int n_orig, int n_out, const int* n, const int* off_l,
                           const int* off_r, const double* eta_l, const double* eta_r, const double* win, const double* delta,
                           int nwin, int index_step, void* stream);

/* ---- f3 packed PCM batches: the sample conversion and channel mean of `librosa.core.load` (src/dataset/upstream_dataset.py:55) and
 * `torchaudio.load` (extras/mast_new/mast/dataloader.py:101), and the window of src/utils/utils.py:166-182, moved behind the upload.
 * pcm = pcm_bytes bytes of interleaved frames in the files' own sample formats; tab [B][4] int64 = {byte offset of the clip's first
 * frame in pcm, frames n, channels C, format (0 u8, 1 s16, 2 s32 - 24-bit files left-justified -, 3 f32)} -> out [B][unit] f32.
 * A sample becomes (x - 128) / 128, x / 2^15, float(x) / 2^31 or itself; a frame is its channels added in float32 in the order of
 * numpy's mean(axis=1) (first to last; C = 8: ((c0+c1)+(c2+c3))+((c4+c5)+(c6+c7))) and divided by C.  align 0: (unit - n) / 2 zeros,
 * the n frames, zeros (the window's centre padding); align 1: the frames first (the fbank batch).  n = 0 gives a row of zeros; the
 * host cuts longer clips at their drawn start, so n <= unit.
 * tab_host (required) is the caller's HOST copy of tab; every row is checked before the launch: format in 0..3, C in 1..8,
 * 0 <= n <= unit, offset a multiple of the sample size, offset + n C size <= pcm_bytes (EINVAL, as for B > 65535 or align not 0 / 1).
 * pcm and out 16-byte aligned and pcm_bytes a multiple of 16 (EALIGN): the mono s16 rows are read in aligned 16-byte chunks that
 * touch the clip, which then never leave [pcm, pcm + pcm_bytes).  16-byte stores when unit % 4 == 0. */
int audiossl_pcm_window(const void* pcm, long pcm_bytes, const long long* tab, const long long* tab_host, float* out, int B,
                        int unit, int align, void* stream);

/* ---- a10 Kmix: src/augmentations/augmentations.py:119-189 (cluster-guided mixup of the finished views) -------------------
 * kmix_cluster: cluster[v] = first argmin_c ||mean_T(views[v]) - centroids[c]|| (centroids [K][F] with unit rows: what
 *   `get_index` computes for the view itself and, once it sits in the memory bank, for the bank entry).
 * kmix_apply: out[v] = log(coef[v][0] e^x + coef[v][1] e^z + eps) with z = ring[slot[v]] (log_mix 0: linear mix; slot < 0:
 *   copy).  Partner choice, the alpha / index draws and the FIFO live on the host (they are numpy-stream exact). */
int audiossl_kmix_cluster(const float* views, const float* centroids, int n_views, int F, int T, int K, int* cluster,
                          void* stream);
int audiossl_kmix_apply(const float* views, const float* ring, const int* slot, const float* coef, int n_views, int n,
                        int log_mix, float* out, void* stream);
int audiossl_mask_fill(float* x, const int* tab, int n_img, int max_masks, int F, int T, int zero_fill, void* stream);

/* ---- K6 stem: src/encoder/audiontt.py:46-50 (features_1) ------------------------------------------------
 * conv1_stats: batch statistics of Conv2d(1,64,3,p=1) output from 54 tap moments (`mom`: 16 x 54 doubles of scratch, the
 *   totals are left in mom[0..53] for the backward); updates running stats; writes scale = gamma*rstd, shift = beta - mean*scale, mean, rstd.
 * conv1_fwd : img [N][F][T] f32 -> pooled [N][T/2][F/2][64] (dtype), conv recomputed, nothing else stored.
 * conv1_bwd : dP (+ dxl [N][F/2*64] / (T/2), may be NULL) -> dW [64][9], dgamma, dbeta (dbias == 0); acc = 32*704
 *             floats of scratch.
 * dtype 0: fp32 VALU convolution, fp32 output (validation path); dtype 2 (forward only): the same convolution, bf16 output
 * (`bf16_hp`).  dtype 1 (forward) / conv_dtype 1 (backward, fp32 gradients): the conv
 * is a bf16 MFMA (taps x weights, K = 9 padded to 16) and so are the nine tap sums of the weight gradient; forward and
 * backward must use the same flavour so the pooling arg-max agrees. */
int audiossl_conv1_stats(const float* img, int N, int F, int T, const float* w, const float* bias, const float* gamma,
                         const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                         double* mom, float* scale, float* shift, float* save_mean, float* save_rstd, void* stream);
/* xl (optional, dtype 1 only): fp32 [AUDIOSSL_CONV1_XL_PARTS][N][F/2 * 64]: four partial sums of the mean over pooled time of
 * `out` (the layer output x_1, audiontt.py:76-78), left by the same launch; tmean3_fwd(x1_parts) adds them in a fixed order -
 * the separate tmean pass re-read the whole pooled map */
#define AUDIOSSL_CONV1_XL_PARTS 4
int audiossl_conv1_fwd(int dtype, const float* img, int N, int F, int T, const float* w, const float* bias,
                       const float* scale, const float* shift, void* out, float* xl, void* stream);
/* Training forward of the bf16 stem in two launches.  A view's MOMENT SLOT is AUDIOSSL_CONV1_MOM_SLOT doubles: [0..53] the 54 tap-moment
 * totals (9 first moments in tap order kh*3+kw, then the 45 second moments of pairs a <= b, row-major upper triangle), followed by 16
 * replica sets of 54 that the moments kernel adds into.
 * conv1_moments_pair: tap moments of img_a and (unless NULL) img_b, both [N][F][T], in ONE launch; `mom` = one slot per view, slot 1
 *   is left alone when img_b is NULL.  Clears the slots it fills unless the caller declared them pre-zeroed; afterwards the replica
 *   sets are filled and [0..53] is still zero.
 * conv1_fwd_train: conv1_finalize + conv1_fwd(dtype 1) in one launch: every workgroup folds the slot's replicas in replica order and
 *   derives scale / shift itself; the first also writes scale, shift, save_mean, save_rstd, the running buffers (may both be NULL)
 *   and the totals to mom[0..53] (conv1_bwd reads them there).  count = N*F*T.  Same bits as the two-launch path given the same
 *   totals. */
#define AUDIOSSL_CONV1_MOM_SLOT (17 * 54)
int audiossl_conv1_moments_pair(const float* img_a, const float* img_b, int N, int F, int T, double* mom, void* stream);
int audiossl_conv1_fwd_train(const float* img, int N, int F, int T, double* mom, double count, const float* w, const float* bias,
                             const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum,
                             float eps, float* scale, float* shift, float* save_mean, float* save_rstd, void* out, float* xl,
                             void* stream);
/* conv1_bwd: dtype = type of the pooled gradient dP (0 fp32, 1 bf16); with conv_dtype 1 (MFMA recompute) dxl stays fp32 whatever
 * dtype says, with conv_dtype 0 dP and dxl share it */
int audiossl_conv1_bwd(int dtype, int conv_dtype, const float* img, int N, int F, int T, const float* w, const float* bias,
                       const float* gamma, const float* scale, const float* shift, const float* mean, const float* rstd,
                       const double* mom, const void* dP, const void* dxl, float* acc, float* dW, float* dbias,
                       float* dgamma, float* dbeta, void* stream);

/* ---- K7/K8 conv blocks 2,3: audiontt.py:52-60, 76-93 ----------------------------------------------------
 * colstats : per-column sum / sum of squares of x [G][M][C] (ld) in fp64 -> [G][C].  `groups` = independent batches that
 *            go through the same layer (the two views of the projector); C % 8 == 0.
 * bn_finalize: train-mode BatchNorm statistics -> per-group scale/shift/mean/rstd [G][C]; running stats (momentum 0.1)
 *            are updated group after group, as the reference's successive module calls do.
 * bn_relu_pool_fwd: Y [N][Ti][Fi][64] -> P [N][Ti/2][Fi/2][64].   tmean_fwd: P -> xl [N][Fo*64] (x_1/x_2/x_3).
 * bn_relu_pool_bwd: dP (+dxl/To) -> dY at every position, dgamma, dbeta (stat = 33*128 floats scratch).
 * im2col3x3 / pack_conv_w / unpack_conv_dw: implicit-GEMM plumbing, tap = kh*3+kw, kh on mel, kw on time. */
int audiossl_colstats(int dtype, const void* x, int groups, long M, int C, long ld, int want_sq, double* sum,
                      double* sumsq, void* stream);
int audiossl_bn_finalize(const double* sum, const double* sumsq, int groups, double count, int C, const float* gamma,
                         const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                         float* scale, float* shift, float* save_mean, float* save_rstd, void* stream);
int audiossl_bn_relu_pool_fwd(int dtype, int ydtype, const void* Y, const float* scale, const float* shift, void* P, int N,
                              int Ti, int Fi, void* stream);
/* bn_finalize + bn_relu_pool_fwd of one train-mode conv block (64 channels) in one launch: every workgroup derives scale / shift
 * from the fp64 sums itself; scale / shift / mean / rstd (for the backward) and the running buffers are written by workgroup 0. */
int audiossl_bn_relu_pool_train_fwd(int dtype, int ydtype, const void* Y, const double* sum, const double* sumsq, int stat_replicas,
                                    double count, const float* gamma, const float* beta, float* running_mean, float* running_var,
                                    float momentum, float eps, void* P, float* scale, float* shift, float* save_mean, float* save_rstd,
                                    int N, int Ti, int Fi, void* stream);
/* BatchNorm + ReLU of a conv block (`audiontt.py:52-60`) on the POOLED raw map that conv3x3_pool_fwd leaves: Praw [N][To][Fo][64]
 * holds per channel the 2x2 window's maximum of the conv output (gamma >= 0) or its minimum (gamma < 0); BN + ReLU is monotone with
 * the sign of gamma, so P = max(0, scale * Praw + shift) equals bn_relu_pool_fwd of the whole conv output.  P may be Praw.
 * bn_relu_pooled_train_fwd starts with the finalisation of bn_relu_pool_train_fwd (same bits); count = N * Ti * Fi of the conv output. */
int audiossl_bn_relu_pooled_fwd(int dtype, const void* Praw, const float* scale, const float* shift, void* P, int N, int To, int Fo,
                                void* stream);
int audiossl_bn_relu_pooled_train_fwd(int dtype, const void* Praw, const double* sum, const double* sumsq, int stat_replicas,
                                      double count, const float* gamma, const float* beta, float* running_mean, float* running_var,
                                      float momentum, float eps, void* P, float* scale, float* shift, float* save_mean,
                                      float* save_rstd, int N, int To, int Fo, void* stream);
int audiossl_tmean_fwd(int dtype, int out_f32, const void* P, void* xl, int N, int To, int Fo, void* stream);
/* x_1, x_2, x_3 of one encoder pass (`audiontt.py:76-93`) in one launch; with P1 == NULL and x1_parts given (out_f32 only)
 * x_1 = sum of the AUDIOSSL_CONV1_XL_PARTS parts conv1_fwd left */
int audiossl_tmean3_fwd(int dtype, int out_f32, const void* P1, void* x1, const float* x1_parts, int To1, int Fo1, const void* P2,
                        void* x2, int To2, int Fo2, const void* P3, void* x3, int To3, int Fo3, int N, void* stream);
int audiossl_bn_relu_pool_bwd(int dtype, int ydtype, int gdtype, const void* Y, const void* dP, const void* dxl, const float* scale,
                              const float* shift, const float* mean, const float* rstd, float* stat, void* dY,
                              float* dgamma, float* dbeta, int N, int Ti, int Fi, void* stream);
/* The same with the statistics pass (dbeta, dgamma) taken from the block's POOLED forward output P [N][Ti/2][Fi/2][64] (activation
 * dtype) instead of a first sweep over Y: the routed gradient lives where P > 0, and there xhat = ((P - shift) / scale - mean) rstd. */
int audiossl_bn_relu_pool_bwd_p(int dtype, int ydtype, int gdtype, const void* Y, const void* P, const void* dP, const void* dxl,
                                const float* scale, const float* shift, const float* mean, const float* rstd, float* stat, void* dY,
                                float* dgamma, float* dbeta, int N, int Ti, int Fi, void* stream);
/* ---- SyncBatchNorm halves (C2: `nn.SyncBatchNorm.convert_sync_batchnorm`, extras/decar-v2/main.py:82).  Every train-mode
 * BatchNorm of the path exists as "sums" + "finalize / apply" with the rank's sums in plain buffers in between, so the caller can
 * all-reduce them (RCCL) and pass the GLOBAL element count:
 *   forward : conv1_moments -> [all-reduce mom[0..53]] -> conv1_finalize;  conv3x3_fwd's sum / sumsq or colstats -> [all-reduce]
 *             -> bn_finalize(count = global)
 *   backward: bn_relu_pool_bwd_stats -> [all-reduce stat[0..127]] -> bn_relu_pool_bwd_apply;  conv1_bwd_sums -> [all-reduce lstat]
 *             -> conv1_bwd_finalize;  colbn_bwd_stats -> [all-reduce tmp] -> colbn_bwd_apply (+ add_d2f of the rank's own sums).
 * Parameter gradients always come from the rank's own sums (the data-parallel gradient all-reduce sums them afterwards).
 * conv1_bwd_finalize's `mom` is the rank's OWN tap-moment totals (what conv1_moments left in mom[0..53] for this rank's images), not
 * the all-reduced ones: they weight the two global means in this rank's share of dW; only `gstat` and `count_global` are global. */
int audiossl_conv1_moments(const float* img, int N, int F, int T, double* mom, void* stream);
int audiossl_conv1_finalize(double* mom_totals, const float* w, const float* bias, const float* gamma, const float* beta,
                            float* running_mean, float* running_var, float momentum, float eps, double count, float* scale,
                            float* shift, float* save_mean, float* save_rstd, void* stream);
int audiossl_conv1_bwd_sums(int dtype, int conv_dtype, const float* img, int N, int F, int T, const float* w, const float* bias,
                            const float* gamma, const float* scale, const float* shift, const float* mean, const float* rstd,
                            const double* mom, const void* dP, const void* dxl, float* acc, float* lstat, void* stream);
int audiossl_conv1_bwd_finalize(const float* acc, const double* mom, const float* w, const float* bias, const float* gamma,
                                const float* mean, const float* rstd, double count_global, const float* gstat, float* dW,
                                float* dbias, float* dgamma, float* dbeta, void* stream);
int audiossl_bn_relu_pool_bwd_stats(int dtype, int ydtype, int gdtype, const void* Y, const void* dP, const void* dxl,
                                    const float* scale, const float* shift, const float* mean, const float* rstd, float* stat,
                                    int N, int Ti, int Fi, void* stream);
int audiossl_bn_relu_pool_bwd_apply(int dtype, int ydtype, int gdtype, const void* Y, const void* dP, const void* dxl,
                                    const float* scale, const float* shift, const float* mean, const float* rstd, float* stat,
                                    const float* gstat, double count_global, void* dY, float* dgamma, float* dbeta, int N, int Ti,
                                    int Fi, void* stream);
int audiossl_colbn_bwd_stats(int dtype, int adtype, int gdtype, const void* a, const void* dh, const float* scale,
                             const float* shift, const float* mean, const float* rstd, int relu, int groups, long M, int C,
                             double* tmp, void* stream);
int audiossl_colbn_bwd_apply(int dtype, int adtype, int gdtype, const void* a, const void* dh, const float* scale,
                             const float* shift, const float* mean, const float* rstd, int relu, int groups, long M, int C,
                             const double* sums, double count, void* da, void* stream);
int audiossl_im2col3x3(int dtype, const void* X, void* col, int N, int Ti, int Fi, void* stream);
int audiossl_pack_conv_w(int dtype, const float* W, void* Wf, void* Wd, void* stream);
/* the two 3x3 layers of one encoder (features_2.0 / features_3.0, audiontt.py:52-60) in one launch */
int audiossl_pack_conv_w2(int dtype, const float* Wa, void* Wfa, void* Wda, const float* Wb, void* Wfb, void* Wdb, void* stream);
int audiossl_unpack_conv_dw(const float* dWp, float* dW, void* stream);

/* Implicit-GEMM 3x3 / 64->64 convolution on the bf16 MFMA pipe (no im2col buffer); bf16 only, Fi in {32, 16}.
 * conv3x3_fwd : Y = conv(X, W) (+bias); W = packed [64][576] (pack_conv_w: Wf = forward, Wd = data gradient);
 *               optional BatchNorm batch statistics of the values as stored: sum / sumsq fp64 [64] (zeroed inside).
 *               stat_replicas > 1: sum -> [stat_replicas][128] doubles (replica r: sums at r*128, sums of squares at r*128 + 64;
 *               sumsq == sum + 64): workgroup i adds into replica i % stat_replicas, bn_relu_pool_train_fwd folds them.
 * conv3x3_wgrad: dWp fp32 [64][576] += dY^T * patches(X) (caller zeroes; unpack_conv_dw maps back to [co][ci][3][3]).
 *   workspace (optional, 256 * 64 * 576 floats = 37.7 MB covers every shape): per-workgroup results are stored there and
 *   folded by a second kernel; null = every workgroup adds its result to dWp with fp32 atomics. */
int audiossl_conv3x3_fwd(const void* X, const void* W, const float* bias, void* Y, int out_f32, double* sum,
                         double* sumsq, int stat_replicas, int N, int Ti, int Fi, void* stream);
/* conv3x3_fwd with the 2x2 max-pool of the following BatchNorm -> ReLU -> MaxPool2d (`audiontt.py:52-60`) taken in its epilogue:
 * Praw [N][Ti/2][Fi/2][64] bf16 = per channel the window's maximum of the stored conv output where gamma[c] >= 0, its minimum where
 * gamma[c] < 0 (bn_relu_pooled_*_fwd turn it into the block's output).  Y bf16 may be NULL: the conv output is then not stored
 * (a forward without a backward).  sum / sumsq as in conv3x3_fwd and required, bit for bit the same values.  Ti must be even. */
int audiossl_conv3x3_pool_fwd(const void* X, const void* W, const float* bias, const float* gamma, void* Y, void* Praw, double* sum,
                              double* sumsq, int stat_replicas, int N, int Ti, int Fi, void* stream);
int audiossl_conv3x3_wgrad(const void* dY, const void* X, float* dWp, float* workspace, long workspace_floats, int N, int Ti,
                           int Fi, void* stream);

/* ---- K9-K12 GEMM: every nn.Linear / matmul / einsum of the path ------------------------------------------
 * (audiontt.py:62-68; delores_s/upstream_expert.py:15-22, 36; delores_m/upstream_expert.py:250-252)
 * C[M,N] (+)= alpha * op(A) * op(B), operands of `dtype`, fp32 accumulate.
 *   trans_a = 0: A is [M][K] (lda)   trans_a = 1: A is [K][M] (lda)
 *   trans_b = 0: B is [N][K] (ldb)   trans_b = 1: B is [K][N] (ldb)     (torch Linear weights are [N][K])
 * The two flags are independent: all four (trans_a, trans_b) combinations are supported by every kernel variant and tested
 * (tests/test_gpu_gemm_matrix.py).  The contiguous dimension of an operand is a multiple of 8, so N % 8 == 0 is required only for
 * trans_b = 1 (M % 8 == 0 only for trans_a = 1, K % 8 == 0 unless both are set); lda / ldb are multiples of 8 and may exceed the width.
 * Epilogue, in order: + bias[N]; ReLU; * keep[M][ldk] * keep_scale (dropout); zero where gate[M][ldg] <= 0;
 * + resid[M][ldr] (fp32, out-of-place residual connection of the transformer blocks; ksplit 1, not atomic);
 * store as dtype, or fp32 (out_f32), or accumulate into fp32 C: atomic = 1 by atomicAdd (required when ksplit > 1 or when
 * other launches may add to C concurrently), atomic = 2 by plain load-add-store (this launch owns C; ksplit 1).
 * ksplit > 1: the bias is added by the first split only; relu / keep / gate need the whole sum and are rejected. */
int audiossl_gemm(int dtype, int trans_a, int trans_b, int M, int N, int K, float alpha, const void* A, long lda,
                  const void* B, long ldb, void* C, long ldc, const float* bias, int relu, const uint8_t* keep, long ldk,
                  float keep_scale, const void* gate, long ldg, int out_f32, int atomic, int ksplit, const float* resid,
                  long ldr, void* stream);

/* bf16 Linear -> ReLU -> Dropout (`src/encoder/audiontt.py:62-66`: fc block of AudioNTT2020Task6) with the keep mask DRAWN in the
 * epilogue: C (bf16) = dropout(relu(alpha op(A) op(B) + bias)) * keep_scale, element (row, col) kept iff the counter hash of
 * audiossl_dropout_mask says so for index row * N + col (seed' = (seed + *counter) mod 2^48; counter nullable) - the same mask, never
 * stored.  The backward gates on the stored output (gate argument of audiossl_gemm), it needs no mask either. */
int audiossl_gemm_dropout(int trans_a, int trans_b, int M, int N, int K, float alpha, const void* A, long lda, const void* B,
                          long ldb, void* C, long ldc, const float* bias, int relu, unsigned long long seed, float p,
                          const long long* counter, float keep_scale, void* stream);

/* `count` (<= 4) independent bf16 problems of one kind in one launch (the three Barlow heads of delores_m): same M,
 * transposes and epilogue (alpha, fp32 / accumulating output, split-K), per-problem N, K, operand pointers and leading
 * dimensions.  N, K, A, lda, B, ldb, C, ldc are HOST arrays of `count` entries. */
int audiossl_gemm_multi(int count, int trans_a, int trans_b, int M, const int* N, const int* K, float alpha,
                        const void* const* A, const long* lda, const void* const* B, const long* ldb, void* const* C,
                        const long* ldc, int out_f32, int atomic, int ksplit, void* stream);
/* gemm_multi whose fp32 results are weight gradients applied on the spot (no reference counterpart: the reference's optimizer.step()
 * reads .grad tensors, `delores_m/upstream_expert.py:306-313`): P[i] / Mom[i] ([M][Nv[i]] fp32, leading dimension ldp[i]) take
 * torch.optim.SGD's update in the epilogue - the arithmetic of audiossl_sgd_momentum bit for bit (common.h: sgd_step) - and
 * Shadow[i] (bf16, nullable) the copy of the new parameter; the gradient itself is never stored.  One K split. */
int audiossl_gemm_multi_sgd(int count, int trans_a, int trans_b, int M, const int* Nv, const int* K, float alpha,
                            const void* const* A, const long* lda, const void* const* B, const long* ldb, float* const* P,
                            float* const* Mom, void* const* Shadow, const long* ldp, float lr, float momentum, float weight_decay,
                            float grad_scale, const float* grad_scale_dev, void* stream);
/* The Barlow-twins cross-correlation of up to four heads with the loss folded into the epilogue (`delores_s/upstream_expert.py:118-131`,
 * `delores_m/upstream_expert.py:266-269`): c_h = alpha * A_h^T B_h, A_h / B_h = the two normalised views [K_h][D] (row-major, K_h =
 * batch rows); stores dc_h = dscale_h * (c_h - I) in bf16 [D][D] and adds coef_h * sum (c_h - I)^2 into loss_rep_h[0..31] (32 fp32
 * replicas the caller zeroes and sums: same-address atomics serialise).  c_h itself is never stored.  D % 64 == 0. */
int audiossl_gemm_multi_barlow(int count, int D, const int* K, float alpha, const void* const* A, const long* lda,
                               const void* const* B, const long* ldb, void* const* dc, const float* coef, const float* dscale,
                               float* const* loss_rep, void* stream);

/* ---- encoder tail: delores_s/upstream_encoder.py:26-28 ---------------------------------------------------- */
int audiossl_maxmean_fwd(int dtype, int out_f32, const void* H, void* y, uint8_t* arg, int N, int Tt, int D, void* stream);
int audiossl_maxmean_bwd(int dtype, int gdtype, const void* dy, const uint8_t* arg, const void* H, void* dA, int N, int Tt,
                         int D, void* stream);

/* ---- ragged batches through the conv encoder, eval mode only (csrc/ragged.hip) --------------------------
 * Clip n of a padded batch has T_n = 1 + lens[n]/hop frames; lens: the batch's int32 [N] sample counts on the device.
 * tail_mask: P [N][To][row_elems] of `dtype`, in place - rows t >= T_n >> shift become zeros with 16-byte stores, rows below are
 *   neither read nor written.  P and a row must be multiples of 16 bytes (EALIGN).
 * tmean3_ragged_fwd: x_l [N][Fo_l*64] fp32 = mean over the first T_n >> l rows of P_l [N][To_l][Fo_l][64], l = 1, 2, 3.
 * meanmax_ragged_fwd: H [N][Tt][D] -> mean [N][D] and maxmean [N][D] = max + mean, fp32, over the first T_n >> shift rows; either
 *   output may be NULL; any Tt (no arg-max is kept: nothing runs backward through it); D % 8 == 0. */
int audiossl_tail_mask(int dtype, void* P, const int* lens, int hop, int shift, int N, int To, long row_elems, void* stream);
int audiossl_tmean3_ragged_fwd(int dtype, const void* P1, float* x1, int To1, int Fo1, const void* P2, float* x2, int To2, int Fo2,
                               const void* P3, float* x3, int To3, int Fo3, const int* lens, int hop, int N, void* stream);
int audiossl_meanmax_ragged_fwd(int dtype, const void* H, float* mean, float* maxmean, const int* lens, int hop, int shift, int N,
                                int Tt, int D, void* stream);

/* ---- K10/K11 Barlow head: delores_s/upstream_expert.py:11-46, src/utils/utils.py:185-189 ------------------
 * colbn_fwd: h = act(scale_g*a+shift_g) on [G][M][C].  colbn_bwd: BatchNorm1d(train) backward per group (tmp = 2*G*C
 * doubles scratch), parameter grads summed over groups.
 * barlow_loss: loss += coef * sum (c - I)^2 ; dc = dscale * (c - I). */
int audiossl_colbn_fwd(int dtype, int adtype, const void* a, const float* scale, const float* shift, int relu, void* h,
                       int groups, long M, int C, void* stream);
/* colbn_train_fwd: colstats + bn_finalize + colbn_fwd of one train-mode BatchNorm1d (`nn.BatchNorm1d` inside the projector,
 * `src/upstream/delores_m/upstream_expert.py:18-29`) in a single launch for short batches (M <= 1024 rows per group,
 * C % 32 == 0): h = act(BN(a)), scale/shift/mean/rstd [G][C] saved for the backward, running statistics updated group
 * after group. */
int audiossl_colbn_train_fwd(int dtype, int adtype, const void* a, const float* gamma, const float* beta,
                             float* running_mean, float* running_var, float momentum, float eps, int relu, int groups,
                             long M, int C, void* h, float* scale, float* shift, float* save_mean, float* save_rstd,
                             void* stream);
int audiossl_colbn_bwd(int dtype, int adtype, int gdtype, const void* a, const void* dh, const float* scale, const float* shift, const float* mean,
                       const float* rstd, int relu, int groups, long M, int C, double* tmp, void* da, float* dgamma,
                       float* dbeta, void* stream);
/* Multi-problem forms (count <= 4 layers of one shape per launch, bf16 outputs) for the three Barlow heads p1-p3 of
 * DeLoRes-M (`src/upstream/delores_m/upstream_expert.py:133-135, 271`), which run the same chain on different operands.
 * The arrays are host arrays of device pointers (null array = null for every problem); stats[p] is [4][groups*C] fp32
 * (scale, shift, mean, rstd), written by the forward and read by the backward.  coef / dscale: host arrays. */
int audiossl_colbn_train_fwd_multi(int count, int adtype, const void* const* a, const float* const* gamma,
                                   const float* const* beta, float* const* running_mean, float* const* running_var,
                                   float momentum, float eps, int relu, int groups, long M, int C, void* const* h,
                                   float* const* stats, void* stream);
int audiossl_colbn_bwd_multi(int count, int adtype, int gdtype, const void* const* a, const void* const* dh,
                             const float* const* stats, int relu, int groups, long M, int C, void* const* da,
                             float* const* dgamma, float* const* dbeta, void* stream);
int audiossl_barlow_loss_multi(int count, const float* const* c, int D, const float* coef, const float* dscale,
                               void* const* dc, float* const* loss_out, void* stream);
int audiossl_add_d2f(const double* src, float* dst, int n, void* stream);
int audiossl_barlow_loss(int dtype, const float* c, int D, float coef, float dscale, void* dc, float* loss_out,
                         void* stream);

/* ---- K12/K13 MoCo head: delores_m/upstream_expert.py:147-172, 231-264, 270 -------------------------------- */
int audiossl_l2norm_fwd(int dtype, const float* q, int B, int D, void* qn, float* qn32, float* inv_norm, void* stream);
/* l2norm_fwd of q and of k and rowdot(qn, kn) * scale in one launch (the MoCo head's prologue) */
int audiossl_moco_prep(int dtype, const float* q, const float* k, int B, int D, float scale, void* qn, float* qn32, float* qinv,
                       void* kn, float* kn32, float* kinv, float* lpos, void* stream);
int audiossl_rowdot(const float* a, const float* b, int B, int D, float scale, float* out, void* stream);
int audiossl_moco_ce_fwd(const float* lpos, const float* lneg, int B, int K, float* lse, float* loss_out, void* stream);
int audiossl_moco_ce_bwd(int dtype, const float* lpos, const float* lneg, const float* lse, int B, int K, float gscale,
                         void* P, float* dlpos, void* stream);
/* The same head without the [B][K] logits in memory (bf16 path): the logits GEMM qn [B][dim] x queue [dim][K] / T reduces
 * its own tile - mode 1: part [B][ceil(K/64)][2] fp32 = (max, sum exp) per 64-column slab; moco_lse_merge folds them with
 * lpos into lse / loss / dlpos; mode 2: P [B][K] bf16 = exp(logit - lse) * gscale, recomputed for the dq GEMM.
 * Replaces `logits = cat([l_pos, l_neg]) / T; F.cross_entropy(logits, 0)` (delores_m/upstream_expert.py:250-264, 270). */
int audiossl_moco_logits(int mode, const void* qn, const void* queue, int B, int K, int dim, float inv_t, float* part,
                         const float* lse, float gscale, void* P, void* stream);
int audiossl_moco_lse_merge(const float* lpos, const float* part, int B, int nslot, float gscale, float* lse,
                            float* loss_out, float* dlpos, void* stream);
int audiossl_l2norm_bwd(int dtype, const float* dqn, const float* dlpos, const float* kn32, const float* qn32,
                        const float* inv_norm, int B, int D, void* dq, void* stream);
/* ptr_dev (optional, int64 on the device = the reference's `queue_ptr` buffer): when given, the write position is read
 * from it and advanced by B (mod K) on the device, so the call can sit inside a captured hipGraph; `ptr` is then ignored. */
int audiossl_enqueue(int dtype, const float* keys, int B, int D, int K, int ptr, long long* ptr_dev, float* queue, void* shadow,
                     void* stream);
/* shadow (optional): bf16 [n], the updated pk as the key encoder's MFMA operands, written in the same pass */
int audiossl_ema_update(float* pk, const float* pq, long n, float m, void* shadow, void* stream);

/* Host-side switch: 1 = every scratch pointer handed to the entry points below is already zero (the caller cleared its whole
 * scratch arena with one memset), so they skip their own hipMemsetAsync; 0 (default) = they zero their scratch themselves. */
int audiossl_set_prezeroed(int on);
/* Host-side query (diagnostics): the kernel the most recent audiossl_gemm / gemm_multi / gemm_multi_barlow / moco_logits call
 * launched, as a substring of the name rocprofv3 prints for it ("gemm_sp_multi_kernel<false, false, 6>"; instantiations on the bf16
 * type appear mangled there: "gemm_multi_kernelIDF16bLb0ELb0ELi64ELi2ELi4E").  The dispatch picks among several instantiations
 * by shape; bench.py's per-kernel roofline table uses this to join its rows to profiles/ kernel_stats.csv.
 * The log-mel entry points and conv3x3_fwd / conv3x3_pool_fwd / conv3x3_wgrad record theirs too ("conv3x3_ws_kernel<32, true, false>",
 * "conv3x3_kernel<16, 4>", "conv3x3_wgrad_kernel<32, 2>+reduce" when the fold of the per-workgroup results follows). */
int audiossl_last_kernel(char* name, int capacity);

/* ---- K17 optimiser + plumbing: delores_s/upstream_expert.py:236-243 (torch.optim.SGD) ---------------------- */
/* sgd_momentum: optional tail work of the same pass - shadow_bf16 (nullable): bf16 copy of the updated parameters (what
 * `cast` would produce at the start of the next step); zero_grad: clear g after reading it. */
int audiossl_sgd_momentum(float* p, float* g, float* buf, long n, float lr, float momentum, float weight_decay,
                          int first, float grad_scale, const float* grad_scale_dev, void* shadow_bf16, int zero_grad,
                          void* stream);
/* sgd_momentum over nseg segments of the flat buffers (segs: DEVICE table of (offset, length) pairs in elements, multiples of 4;
 * max_n = the longest; shadow_bf16 nullable, indexed like p): the remaining tensors of a slice whose large ones gemm_multi_sgd updated. */
int audiossl_sgd_momentum_segments(float* p, float* g, float* buf, const long* segs, int nseg, long max_n, float lr, float momentum,
                                   float weight_decay, int first, float grad_scale, const float* grad_scale_dev, void* shadow_bf16,
                                   int zero_grad, void* stream);
/* g[segs[2s] .. + segs[2s+1]) = 0 for nseg segments (segs: DEVICE table of (offset, length) pairs in elements, max_n = the longest):
 * clears the small tensors of a flat gradient whose large ones are stored, not accumulated, by their single writer
 * (src/optim.py: HipSGD.step_tail(keep_stale=...)); no reference counterpart - the reference's optimizer.zero_grad() clears all. */
int audiossl_zero_segments(float* g, const long* segs, int nseg, long max_n, void* stream);
int audiossl_cast(int dtype, const float* src, void* dst, long n, void* stream);
int audiossl_cast_back(int dtype, const void* src, float* dst, long n, void* stream);
/* keep[i] = splitmix64(seed', i) >= p; seed' = (seed + *counter) mod 2^48 when `counter` (device int64) is given, so that
 * a replayed hipGraph draws a fresh mask every step. */
int audiossl_dropout_mask(uint8_t* keep, long n, unsigned long long seed, float p, const long long* counter, void* stream);
/* out = g where h > 0 else 0 (nn.ReLU backward on the stored activation); eval-mode BatchNorm folded to scale/shift
 * (audiontt.py:47,53,58 under model.eval()); y += a*x on fp32 buffers. */
int audiossl_relu_bwd(int dtype, const void* g, const void* h, void* out, long n, void* stream);
int audiossl_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                            float eps, int C, float* scale, float* shift, void* stream);
int audiossl_axpy(float* y, const float* x, float a, long n, void* stream);
/* x = hi + lo, hi = bf16(x), lo = bf16(x - hi): the projector's first GEMM runs on both pieces, because the time-pooled
 * features it reads have |mean| >> batch-std and a single bf16 rounding would eat their batch variation. */
int audiossl_split_bf16(const float* x, void* hi, void* lo, long n, void* stream);
/* Default bf16 path, same problem at no extra GEMM: yc = bf16(y - column mean per group) [G][M][C], cmean [G][C] fp32
 * (M <= 1024, C % 32 == 0).  The projector's first Linear has no bias and is followed by train-mode BatchNorm
 * (`src/upstream/delores_s/upstream_expert.py:15-22`), which removes the per-column constant the shift produces; the weight
 * gradient is unchanged because a BatchNorm input gradient sums to zero over the batch.  shift_running_mean repairs the
 * one thing that does see the shift: running_mean[j] += sum_g m (1-m)^(G-1-g) cmean[g] . W[j]   (W bf16 [D][K]). */
int audiossl_center_cast(const float* y, void* yc, float* cmean, int groups, long M, int C, void* stream);
int audiossl_shift_running_mean(const void* W, const float* cmean, float* running_mean, int D, int K, int groups,
                                float momentum, void* stream);
/* the same for up to four heads per launch (host arrays of device pointers / widths, as the other *_multi entry points) */
int audiossl_center_cast_multi(int count, const float* const* y, void* const* yc, float* const* cmean, const int* C, int groups,
                               long M, void* stream);
int audiossl_shift_running_mean_multi(int count, const void* const* W, const float* const* cmean, float* const* running_mean,
                                      int D, const int* K, int groups, float momentum, void* stream);

/* ---- K14 NT-Xent / ClusterLoss: extras/slicer/contrastive_loss.py:6-92 -----------------------------------------
 * sim [N][N] fp32 = z z^T / tau from audiossl_gemm (N = 2B; positives at (r + B) mod N; the diagonal is excluded).
 * fwd: lse[r] and loss += mean_r(lse_r - sim[r][pos]).  bwd: dsim = (softmax - onehot_pos) * gscale, 0 on the diagonal. */
int audiossl_ntxent_fwd(const float* sim, int N, int B, float* lse, float* loss_out, void* stream);
int audiossl_ntxent_bwd(int dtype, const float* sim, const float* lse, int N, int B, float gscale, void* dsim, void* stream);

/* ---- K15/K16 DeepCluster-v2: extras/decar-v2/utils.py:291-318 (k-means E/M steps), main.py:228-233 (prototype CE) ----
 * row_argmax: assign[r] = first argmax of dot[r][:] (dot = mem * centroids^T from audiossl_gemm).
 * kmeans_accumulate: sums[a] += x[r], counts[a] += 1 (zeroed inside).  kmeans_update: mean + L2-normalise, empty
 * clusters keep their previous centroid.  ce_rows: CrossEntropyLoss(ignore_index) forward + dlogits. */
int audiossl_row_argmax(const float* dot, long N, int K, long long* assign, void* stream);
int audiossl_kmeans_accumulate(const float* x, const long long* assign, long N, int K, int D, float* sums, int* counts,
                               void* stream);
int audiossl_kmeans_update(const float* sums, const int* counts, int K, int D, float* centroids, void* stream);
/* Offline pseudo-labeler (extras/decar-v2/clustering.py:19-115: faiss PCA-whitening + k-means): the Lloyd M step with plain
 * means (empty clusters keep their centroid) and out[r] = scale * |x_r|^2, the bias that turns the dot-product GEMM + row_argmax
 * into the Euclidean E step. */
int audiossl_kmeans_update_mean(const float* sums, const int* counts, int K, int D, float* centroids, void* stream);
int audiossl_row_sqnorm(const float* x, int rows, int D, float scale, float* out, void* stream);
int audiossl_ce_rows(int dtype, const float* logits, const long long* target, int B, int K, int ignore_index, int* cnt,
                     float* loss_out, void* dlogits, void* stream);

/* ---- K19 UnFuSeD self-distillation loss: src/upstream/unfused/upstream_expert.py:141-168, src/utils/utils.py:191-197
 * (original extras/unfused/moco_model.py:286-342).  z1..z3 (students) and t (teacher): fp32 [B][ld] logits, ld >= C,
 * ld % 4 == 0, columns [C, ld) never used (they may hold NaN); label int64 [B].
 *   loss4 += {total, CE, KL, MSE}:  CE = alpha sum_h mean CE(z_h, y) + mean CE(t, y),
 *                                   KL = beta sum_h batchmean KL(softmax(t) || softmax(z_h))  (target NOT detached),
 *                                   MSE = gamma sum_h mean (2 - 2 cos(z_h, t))  (F.normalize eps 1e-12).
 * dz1..dz3, dt: gradients in the same [B][ld] layout, fp32 (gdtype 0) or bf16 (gdtype 1), columns [C, ld) written as zeros;
 * all four NULL = forward only, any mixture is EINVAL.  2 <= C <= 4096 (a row's four vectors live in one workgroup's
 * registers).  A label outside [0, C) is never used as an index and adds NaN to all four loss slots.  One launch. */
int audiossl_unfused_loss(int gdtype, const float* z1, const float* z2, const float* z3, const float* t,
                          const long long* label, int B, int C, long ld, float alpha, float beta, float gamma,
                          float* loss4, void* dz1, void* dz2, void* dz3, void* dt, void* stream);

/* ---- K20 k-NN evaluation on frozen embeddings (csrc/knn.hip).  No counterpart runs in the reference: its `validation_step`s
 * import `precision_at_k` and stop there; this is the weighted k-NN classifier of InstDisc / MoCo / DINO (`knn_classifier`,
 * DINO eval_knn.py) and replaces `sim = q @ bank.T; sim.topk(k)` plus the one-hot scatter / exp(sim / T) vote after it.
 * knn_topk: q [Nq][D], bank [Nb][D] row-major bf16 (the caller normalises: audiossl_l2norm_fwd writes such rows), fp32
 *   accumulation on the MFMA pipe.  top_sim / top_idx [Nq][k]: each query's k largest dot products in descending order and
 *   their bank rows, equal values by ascending row.  The [Nq][Nb] matrix is never stored; `workspace` (device,
 *   audiossl_knn_workspace bytes, needs no clearing) holds the per-split partial lists when the bank is split over workgroups.
 *   1 <= k <= 128, k <= Nb < 2^31, Nq >= 1, D % 32 == 0, 32 <= D <= 4096; inputs finite.
 * knn_workspace (host): bytes for knn_topk, O(Nq k splits), non-decreasing in Nq and in k.
 * knn_vote: neighbour j weighs exp((top_sim[j] - row max) * inv_t) (inv_t = 0: majority vote); pred = the int64 label
 *   (bank_label[top_idx[j]], compared only, never an index) with the largest summed weight, ties to the smaller label; conf = that
 *   sum / the row's total.  A row with a top_idx outside [0, Nb) reads no label and gets pred = -1, conf = NaN. */
int audiossl_knn_workspace(int Nq, long Nb, int k, long* bytes);
int audiossl_knn_topk(const void* q, const void* bank, int Nq, long Nb, int D, int k, float* top_sim, int* top_idx,
                      void* workspace, long workspace_bytes, void* stream);
int audiossl_knn_vote(const float* top_sim, const int* top_idx, const long long* bank_label, int Nq, int k, long Nb,
                      float inv_t, long long* pred, float* conf, void* stream);

/* ---- K21 centred kernel alignment between two feature sets of the same n clips (csrc/cka.hip): `linear_CKA` / `kernel_CKA`
 * of extras/CKA.py:1-60, without its n x n matrices.  x [n][p], y [n][q] row-major fp32, row i of both from the same clip;
 * 2 <= n <= 65536, p and q multiples of 4 in [4, 4096] (pad with zero columns: they change no Gram entry).  Gram tiles on the
 * fp32-input MFMA, reduced where they are formed: sum(HKH * HLH) = S_KL - (2/n) sum_i k_i l_i + k l / n^2 (k_i, l_i row sums,
 * k, l totals), fp64 sums folded in a fixed order, so two calls agree bit for bit.  Nothing synchronises with the host.
 * cka_workspace (host): bytes of `workspace` for cka_sigma2 and cka_hsic, non-decreasing in n; it needs no clearing.
 * cka_center: out = x - column mean (fp64 means, one rounding); changes neither the centred linear Gram nor any distance.
 *   cka_sigma2 and cka_hsic take the data as given.
 * cka_sigma2: sigma2[0] = median of the non-zero d_ij = max((g_ii + g_jj) - 2 g_ij, 0) over j > i (equal to the median over the
 *   full symmetric matrix, `np.median(KX[KX != 0])`): the mean of the order statistics (M-1)/2 and M/2 of the kernel's own fp32
 *   distances, exact (radix select over their bit patterns, three sweeps); count[0] (optional) = M.  M = 0 gives NaN.
 * cka_hsic: kernel 0 = linear (K = X X^T), 1 = RBF (K_ij = exp(-d_ij / (2 sigma^2)), d_ii = 0, the coefficient -0.5 / sigma^2
 *   formed in fp64 and rounded to fp32 once).  RBF takes EITHER sigma > 0 for both matrices (sigma2_x = sigma2_y = NULL) OR both
 *   device pointers sigma2_x, sigma2_y (as cka_sigma2 wrote them) with sigma = 0.  out[8] (device, fp64) = {cka, hsic_xy,
 *   hsic_xx, hsic_yy, S_kl, S_kk, S_ll, 0}; rowsum_k / rowsum_l [n] fp64 are optional outputs (NULL = not wanted). */
int audiossl_cka_workspace(int n, int p, int q, long* bytes);
int audiossl_cka_center(const float* x, int n, int p, float* out, void* stream);
int audiossl_cka_sigma2(const float* x, int n, int p, double* sigma2, long long* count, void* workspace,
                        long workspace_bytes, void* stream);
int audiossl_cka_hsic(const float* x, const float* y, int n, int p, int q, int kernel, double sigma,
                      const double* sigma2_x, const double* sigma2_y, double* out, double* rowsum_k,
                      double* rowsum_l, void* workspace, long workspace_bytes, void* stream);

/* ---- K23 power-iteration clustering on an exact nearest-neighbour graph (csrc/graph.hip): `make_graph`, `make_adjacencyW`,
 * `run_pic` and `find_maxima_cluster` of extras/decar-v2/clustering.py:118-230 (faiss index, scipy csr_matrix and Python loops
 * there).  Every workspace is device memory that needs no clearing; two calls on the same inputs agree bit for bit (no float
 * atomics); nothing synchronises with the host.
 * knn_graph_l2: x [n][d] row-major fp32 -> idx [n][k] int32, d2 [n][k] fp32: for each row i the k rows j != i with the smallest
 *   d2_ij = max(0, (n_i + n_j) - 2 g_ij), in the order (d2 ascending, j ascending) - a strict total order, so heavy ties are
 *   resolved the same way however the tiles are walked.  g_ij on the fp32-input MFMA, an fmaf chain over d in index order;
 *   n_i = g_ii by the same chain, so a repeated row is at distance exactly 0.  Self is excluded by index: a duplicate row IS a
 *   neighbour.  The n x n matrix is never stored.  1 <= k <= 64, k <= n - 1, d % 4 == 0 (pad with zero columns), 4 <= d <= 4096,
 *   n k < 2^31; inputs finite.
 * knn_graph_workspace (host): bytes for knn_graph_l2 (norms + per-split lists), non-decreasing in n and in k.
 * pic_build: idx, d2 [n][k] as knn_graph_l2 wrote them (a row's entries distinct; an index outside [0, n) is dropped), sigma > 0 ->
 *   CSR of W = A + A^T, A_ij = exp(-d2_ij / sigma^2) for j in row i's list, exponent and exp in fp64.  rowptr [n + 1], col and
 *   w [2 n k] (capacity; nnz[0] entries are written), rows canonical: columns ascending, a mutual pair merged into one entry
 *   a_ij + a_ji.  Any in-degree up to n - 1.  n k < 2^30.
 * pic_power: v [n] fp64 = `iters` rounds of u = alpha W v + (1 - alpha) / n, v = u / sum(u), from v = 1 / n.  Row sums in column
 *   order, the global sum in a fixed tree.  `cap` = entries col / w hold (rowptr is clamped to it, a column outside [0, n) is
 *   skipped: a malformed matrix cannot make the kernels read out of bounds).
 * pic_assign: parent(i) = the neighbour j maximising W_ij (v_j - v_i) among strictly positive values, ties to the smaller j,
 *   else i; label[i] = number of its root among the roots in ascending node order, count[0] = number of roots.  Roots by
 *   pointer doubling, ceil(log2 n) rounds.
 * pic_workspace (host): bytes that serve pic_build (n, k), pic_power and pic_assign (n). */
int audiossl_knn_graph_workspace(int n, int k, long* bytes);
int audiossl_knn_graph_l2(const float* x, int n, int d, int k, int* idx, float* d2, void* workspace, long workspace_bytes,
                          void* stream);
int audiossl_pic_workspace(int n, int k, long* bytes);
int audiossl_pic_build(const int* idx, const float* d2, int n, int k, double sigma, int* rowptr, int* col, double* w, int* nnz,
                       void* workspace, long workspace_bytes, void* stream);
int audiossl_pic_power(const int* rowptr, const int* col, const double* w, int n, long cap, double alpha, int iters, double* v,
                       void* workspace, long workspace_bytes, void* stream);
int audiossl_pic_assign(const int* rowptr, const int* col, const double* w, const double* v, int n, long cap, int* label,
                        int* count, void* workspace, long workspace_bytes, void* stream);

/* ---- exact range search and connected components (csrc/range.hip): every pair of rows closer than a radius - near-duplicates
 * inside one file list, leakage between two; faiss `range_search` in the reference's stack.  The output length is not known before
 * the launch: range_count, one host read of `total`, range_fill.  Every workspace is device memory that needs no clearing; two
 * calls on the same inputs agree bit for bit (no float atomics); nothing synchronises with the host.  Every entry returns EINVAL for
 * a null pointer or a refused shape before any launch, EALIGN for x or a workspace that is not 16-byte aligned.
 * range_workspace (host): bytes for range_count / range_fill (the norms of all n rows + the per-(row, split) counts), non-decreasing
 *   in each argument: a workspace sized for a forced `splits` also serves splits = 0.  1 <= rows <= n, 0 <= splits <= 64.
 * range_count: x [n][d] row-major fp32, d % 4 == 0 (pad with zero columns), 4 <= d <= 4096; owned rows [own_lo, own_hi), walked
 *   rows [walk_lo, walk_hi), both non-empty and inside [0, n); r2 >= 0 and finite.  For every owned row i it counts the walked
 *   rows j != i with d2_ij <= r2, d2_ij = max(0, (n_i + n_j) - 2 g_ij): knn_graph_l2's arithmetic (fp32-input MFMA, an fmaf chain
 *   over d in index order, n_i = g_ii by the same chain), so a repeated row is at distance exactly 0 and d2_ij == d2_ji bit for
 *   bit.  i == j leaves by index: a duplicate row IS a match.  rowptr [rows + 1] int32, rows = own_hi - own_lo: the exclusive scan
 *   of the counts, formed on the device.  total [1] (64-bit, 8-byte aligned): the true number of matches, also when it does not
 *   fit int32 - rowptr is then unspecified and the caller must refuse.  splits: 0 = the library chooses how many workgroups share
 *   one 64-row block's walk (few rows must not leave the chip idle), 1..64 forces it (capped at the number of 128-row tiles).
 * range_fill: the same geometry, r2 and splits, and the workspace range_count left; `total` as read from range_count.  col [cap]
 *   int32 = the ABSOLUTE row index j, d2 [cap] fp32; row i's entries at rowptr[i] .., in ascending j - a strict order, so the
 *   result does not depend on splits or on how tiles are walked.  cap < total, total < 0 or total >= 2^31: EINVAL, nothing is
 *   written.  Entries at or past `total` are not written (every store is bounded by it on the device as well).
 * graph_components: weakly connected components of a CSR graph on n >= 1 nodes: an entry (i, j) links i and j whether or not
 *   (j, i) is stored.  `cap` = entries col holds (rowptr [n + 1] is clamped to it, a column outside [0, n) is skipped, as in
 *   pic_power).  label [n] int32 = the number of i's component when components are ordered by their smallest member (pic_assign's
 *   convention), count [0] = the number of components.  One hook kernel (integer compare-and-swap, larger root under smaller: the
 *   fixed point is unique, so the result is deterministic) and ceil(log2 n) rounds of pointer doubling.
 * graph_components_workspace (host): bytes for graph_components, non-decreasing in n. */
int audiossl_range_workspace(int n, int rows, int splits, long* bytes);
int audiossl_range_count(const float* x, int n, int d, int own_lo, int own_hi, int walk_lo, int walk_hi, float r2, int splits,
                         int* rowptr, long long* total, void* workspace, long workspace_bytes, void* stream);
int audiossl_range_fill(const float* x, int n, int d, int own_lo, int own_hi, int walk_lo, int walk_hi, float r2, int splits,
                        const int* rowptr, long long total, int* col, float* d2, long cap, void* workspace, long workspace_bytes,
                        void* stream);
int audiossl_graph_components_workspace(int n, long* bytes);
int audiossl_graph_components(const int* rowptr, const int* col, int n, long cap, int* label, int* count, void* workspace,
                              long workspace_bytes, void* stream);

/* ---- exact minimum spanning tree of the complete mutual-reachability graph (csrc/mst.hip): the stage of HDBSCAN (Campello et al.
 * 2013; sklearn.cluster.HDBSCAN) that a neighbour list cannot give - single linkage over every threshold at once.  The n x n
 * matrix is never stored: Boruvka's algorithm, one pass over the Gram tiles per round, ceil(log2 n) rounds issued, every kernel of
 * a round returning at once when one component is left.  The workspace is device memory that needs no clearing; two calls on the
 * same inputs agree bit for bit (integer atomic minima only, no float atomics); nothing synchronises with the host.  EINVAL for a
 * null pointer or a refused shape before any launch, EALIGN for x or a workspace that is not 16-byte aligned.
 * mreach_mst_workspace (host): bytes for mreach_mst (norms, component arrays, per-(row, split) candidates), non-decreasing in each
 *   argument: a workspace sized for a forced `splits` also serves splits = 0.  n >= 2, 0 <= splits <= 64.
 * mreach_mst: x [n][d] row-major fp32, n >= 2, d % 4 == 0 (pad with zero columns), 4 <= d <= 4096; core2 [n] fp32 >= 0, or NULL for
 *   all zeros (the plain Euclidean tree); inputs finite.  Edge weights w2_ij = max(d2_ij, core2_i, core2_j), d2_ij = max(0, (n_i +
 *   n_j) - 2 g_ij): knn_graph_l2's and range_fill's arithmetic (fp32-input MFMA, an fmaf chain over d in index order, n_i = g_ii by
 *   the same chain), so d2_ij == d2_ji bit for bit and a core2 taken from knn_graph_l2's d2 ties bit for bit with the matching
 *   d2_ij.  Edges are compared by the strict total order (w2 bits, min(i, j), max(i, j)): the tree is unique however heavy the
 *   ties (repeated rows, integer data, core distances that dominate), it is Kruskal's under that order, and it does not depend on
 *   `splits` or on how the tiles are walked.  eu, ev [n - 1] int32 with eu < ev, ew2 [n - 1] fp32: the edges, rounds in order and
 *   inside a round by the id of the component that chose the edge - deterministic, not sorted.  rounds [1] (may be NULL): the
 *   number of Boruvka rounds that did work.  splits: 0 = the library chooses how many workgroups share one 64-row block's walk,
 *   1..64 forces it (capped at the number of 128-row tiles). */
int audiossl_mreach_mst_workspace(int n, int splits, long* bytes);
int audiossl_mreach_mst(const float* x, int n, int d, const float* core2, int splits, int* eu, int* ev, float* ew2, int* rounds,
                        void* workspace, long workspace_bytes, void* stream);

/* ---- label spreading on the same graph (csrc/spread.hip): Zhou et al. 2004, sklearn's `LabelSpreading`; the reference has no
 * counterpart.  S = D^-1/2 W D^-1/2, F_0 = Y, F <- alpha S F + (1 - alpha) Y on an [n][m] block whose m columns are independent
 * problems (classes x trials of a low-shot evaluation).  No float atomics: two calls agree bit for bit, and a column's result
 * does not depend on which other columns share the call; the workspace needs no clearing; nothing synchronises with the host.
 * Every entry returns EINVAL for a null pointer before any launch.
 * spread_workspace (host): bytes for spread_run (the second F buffer), non-decreasing in n and in m; refuses what spread_run does.
 * spread_normalize: the CSR of pic_build (`cap` = entries col / w / s hold; rowptr is clamped to it, a column outside [0, n) gives
 *   s = 0 and adds nothing to deg) -> deg [n] fp64 = row sums in column order; s [cap] fp32, s_l = (float)(w_l / sqrt(deg_i deg_j))
 *   for entry l = (i, j), product, root and quotient in fp64: s_ij == s_ji bit for bit.  A zero product gives s_l = 0 (a node whose
 *   weights all underflowed): no inf, no NaN.  Entries no row points at are not written.  n >= 2, cap >= 0.
 * spread_run: Y is never stored: Y[i][seed_col[q]] = 1 for q in seed_ptr[i] .. seed_ptr[i + 1] - 1 (seed_ptr [n + 1], clamped to
 *   `seeds`; a seed_col outside [0, m) is skipped).  f [n][m] fp32 = F after `iters` rounds; fp32 storage, every value one fmaf
 *   chain over its row's entries in column order, then fmaf(alpha, sum, (1 - alpha) Y).  A column outside [0, n) is skipped.
 *   n >= 2, 4 <= m <= 16384, m % 4 == 0 (pad with empty columns), n m < 2^31, 0 < alpha < 1, 1 <= iters <= 10^6, seeds >= 0,
 *   cap >= 0, workspace_bytes >= spread_workspace (EINVAL); f and workspace 16-byte aligned (EALIGN).
 * spread_assign: f [n][ldf]; trial t owns columns t classes .. (t + 1) classes - 1.  label [n][trials] = arg-max over them, ties to
 *   the lowest class, -1 when the largest value is <= 0 (unreached).  confidence [n][trials] fp32 = 1 - H(p) / log(classes),
 *   p = row / sum(row) over the positive entries (Iscen et al. 2019, eq. 11), in fp64 from the fp32 row; 0 for an unreached row,
 *   else 1 when classes == 1.  n, classes, trials >= 1, classes trials <= ldf, n ldf < 2^31. */
int audiossl_spread_workspace(int n, int m, long* bytes);
int audiossl_spread_normalize(const int* rowptr, const int* col, const double* w, int n, long cap, double* deg, float* s,
                              void* stream);
int audiossl_spread_run(const int* rowptr, const int* col, const float* s, int n, long cap, const int* seed_ptr,
                        const int* seed_col, int seeds, int m, double alpha, int iters, float* f, void* workspace,
                        long workspace_bytes, void* stream);
int audiossl_spread_assign(const float* f, int n, int ldf, int classes, int trials, int* label, float* confidence, void* stream);

/* ---- silhouette coefficient of a labeling on its features (csrc/silhouette.hip): sklearn's `silhouette_samples`, Euclidean -------
 * The label-free score of a pseudo-labeling (`store_clusters --score`, `--k_sweep`); the reference has no counterpart.
 * silhouette: xs [n][d] row-major fp32, rows SORTED BY CLUSTER; seg [K + 1] int32 offsets (device): cluster c is rows seg[c] ..
 *   seg[c + 1] - 1; seg_host = the caller's host copy of seg, checked before any launch.  s [n] fp64, in the sorted order:
 *     a_i = mean distance to the other members of i's cluster, b_i = min over the other clusters of the mean distance to their
 *     members, s_i = (b_i - a_i) / max(a_i, b_i); s_i = 0 when i's cluster has one member and for 0 / 0.
 *   dist_ij = sqrt(max(0, (n_i + n_j) - 2 g_ij)): g_ij and n_i = g_ii by knn_graph_l2's chain (fp32-input MFMA, d in index order),
 *   so a repeated row is at distance exactly 0; (i, i) leaves by index; the fp32 sqrt is correctly rounded; every sum of
 *   distances, the means, the min and the quotient are fp64.  Neither the n x n matrix nor an n x K table is stored: one
 *   workgroup per 64 rows walks all columns and folds a cluster's sum when its last column has passed.  No atomics; the workspace
 *   (n norms) needs no clearing; two calls agree bit for bit; nothing synchronises with the host.
 *   n >= 3, d % 4 == 0 (pad with zero columns), 4 <= d <= 4096, 2 <= K <= n - 1, seg_host[0] == 0, seg_host[K] == n, every
 *   segment non-empty (EINVAL); xs and workspace 16-byte aligned (EALIGN); inputs finite.
 * silhouette_workspace (host): bytes for silhouette, non-decreasing in n. */
int audiossl_silhouette_workspace(int n, long* bytes);
int audiossl_silhouette(const float* xs, int n, int d, const int* seg, const int* seg_host, int K, double* s, void* workspace,
                        long workspace_bytes, void* stream);

/* ---- t-SNE map of a feature matrix (csrc/tsne.hip): van der Maaten & Hinton 2008 with the parameters and schedule of
 * `sklearn.manifold.TSNE`: sparse affinities on each point's nearest neighbours (its `barnes_hut` path), EXACT repulsion (what
 * `angle = 0` would give); the reference has no counterpart.  Nothing holds n x n numbers; no float atomics: two calls on the same
 * inputs agree bit for bit; every workspace is device memory that needs no clearing; nothing synchronises with the host.
 * Every entry returns EINVAL for a null pointer, n < 2 or k outside [1, 64] before any launch.
 * tsne_calibrate: d2 [n][k] fp32 as knn_graph_l2 wrote it -> p_cond [n][k] fp32, p_j|i = exp(-beta_i (d2_ij - min_t d2_it)) / sum,
 *   and beta [n] fp32.  beta_i by the bisection of `_binary_search_perplexity` (sklearn/manifold/_utils.pyx): from 1, doubled or
 *   halved while a bound is infinite, then the midpoint, at most 100 steps, until |H_i - log(perplexity)| <= 1e-5 with
 *   H_i = -sum_j p_j|i log p_j|i of the row as it is stored (fp32), so the stored row meets the tolerance itself; search,
 *   exponentials, logs and sums in fp64.  A row of equal distances ends as the uniform
 *   row 1 / k.  0 < perplexity <= k, k <= n - 1, n k < 2^30; distances finite.
 * tsne_symmetrize: idx [n][k] int32 (a row's entries distinct, no self; an index outside [0, n) is dropped), p_cond [n][k] ->
 *   CSR of P = (P_cond + P_cond^T) / (2 n): rowptr [n + 1] int32, col int32 and p fp32 [2 n k] (capacity; nnz[0] entries are
 *   written), columns ascending in every row, a mutual pair merged into one entry (the two terms added in fp64, rounded once).
 * tsne_repulsion: y [n][2] fp32 -> rep [n][2] fp32, rep_i = sum_{j != i} w_ij^2 (y_i - y_j), and Z[0] (device, fp64) =
 *   sum_{i != j} w_ij with w_ij = 1 / (1 + |y_i - y_j|^2).  All n (n - 1) pairs; (i, i) leaves by index, a coincident point
 *   contributes w = 1 and force 0.  fp32 terms (1 / x within an ulp of the rounded quotient), fp32 sums over one 256-point tile,
 *   fp64 across tiles and splits, folded in a fixed order.  |y| < 1e18.
 * tsne_gradient: the CSR (cap = entries col / p hold; rowptr is clamped to it and a column outside [0, n) is skipped), y, rep and Z
 *   as tsne_repulsion wrote them -> grad [n][2] fp32 = 4 (exaggeration att_i - rep_i / Z), att_i = sum_j p_ij w_ij (y_i - y_j)
 *   over row i, and kl[0] (device, fp64; NULL = not wanted, workspace may then be NULL) = sum_ij p_ij log(p_ij Z / w_ij) of the
 *   UNexaggerated P, log and sum in fp64, folded in a fixed order.
 * tsne_update: `_gradient_descent` of sklearn/manifold/_t_sne.py on every element, fp32, in place: inc = update grad < 0;
 *   gains = max(inc ? gains + 0.2 : gains 0.8, 0.01); update = momentum update - learning_rate gains grad; y += update.
 * y, rep and grad 8-byte aligned, workspaces 16-byte aligned (EALIGN).
 * tsne_workspace (host): bytes that serve tsne_symmetrize (n, k), tsne_repulsion and tsne_gradient (n). */
int audiossl_tsne_workspace(int n, int k, long* bytes);
int audiossl_tsne_calibrate(const float* d2, int n, int k, double perplexity, float* p_cond, float* beta, void* stream);
int audiossl_tsne_symmetrize(const int* idx, const float* p_cond, int n, int k, int* rowptr, int* col, float* p, int* nnz,
                             void* workspace, long workspace_bytes, void* stream);
int audiossl_tsne_repulsion(const float* y, int n, float* rep, double* Z, void* workspace, long workspace_bytes, void* stream);
int audiossl_tsne_gradient(const int* rowptr, const int* col, const float* p, long cap, const float* y, const float* rep,
                           const double* Z, int n, double exaggeration, float* grad, double* kl, void* workspace,
                           long workspace_bytes, void* stream);
int audiossl_tsne_update(const float* grad, int n, double momentum, double learning_rate, float* y, float* update, float* gains,
                         void* stream);

/* ---- K22 audio tagging (multi-label downstream, csrc/tagging.hip): nn.BCEWithLogitsLoss (the "bce_logit" of
 * `extras/mast_new/mast/mvit/models/losses.py:38`) on the multi-hot / mixed targets of `mast/dataloader.py:157-184` and the per-class metrics of
 * `extras/mast_new/mast/utilities/stats.py:11-57` (sklearn's average_precision_score / roc_auc_score, class by class on the host
 * there).
 * bce_rows: logits, targets fp32 [N][C], targets in [0, 1] (soft after a mix).  loss_out[0] (one float32, written, not
 *   accumulated) = mean over N*C of max(x,0) - x t + log1p(exp(-|x|)): fp32 terms, fp64 sum in a fixed order by one workgroup
 *   (the entry point takes no scratch), no atomics - two calls agree bit for bit.  dlogits [N][C] fp32 (dtype 0) or bf16
 *   (dtype 1) = (sigmoid(x) - t) / (N*C); NULL = forward only.  N >= 1, C >= 1, N*C <= 2^40.
 * tagging_stats: scores fp32 [N][C] (finite; raw logits rank at least as finely as their sigmoid), targets uint8 [N][C]
 *   (non-zero = positive).  Per class c:
 *     npos[c]     = number of positives;
 *     auc_num2[c] = sum over positives i of 2 #{negatives j: s_j < s_i} + #{negatives j: s_j == s_i}  (exact integer);
 *     auc[c]      = auc_num2 / (2 npos nneg): roc_auc_score, ties at half credit (the ROC trapezoid over tie groups);
 *     ap[c]       = (1/npos) sum over positives i of #{positives j: s_j >= s_i} / #{all j: s_j >= s_i}: average_precision_score
 *                   (thresholds = distinct scores, a tie group's recall step at the precision after the whole group).
 *   ap and auc are NaN for a class without a positive or without a negative (auc_num2 is then 0).  +0.0 and -0.0 are one tie
 *   group.  No sort: integer pair counts of each class's positives against its column, then one fp64 sum per class in a fixed
 *   order (no float atomics), so the outputs depend on the inputs alone.  Work ~ sum_c npos_c (N + npos_c) comparisons.
 *   `workspace` (device, tagging_workspace bytes) holds the class-major copies, the compacted positives and the per-workgroup
 *   partials; it needs no clearing.  1 <= N < 2^31, C >= 1, C * N <= 2^40 and C * ceil(N / 256) < 2^31; `scores` and
 *   `workspace` 16-byte aligned.  Nothing synchronises with the host.
 * tagging_workspace (host): bytes for tagging_stats, about 9 C N + 16 C ceil(N / 256), non-decreasing in N and in C. */
int audiossl_bce_rows(int dtype, const float* logits, const float* targets, long N, int C, float* loss_out, void* dlogits,
                      void* stream);
int audiossl_tagging_workspace(long N, int C, long* bytes);
int audiossl_tagging_stats(const float* scores, const unsigned char* targets, long N, int C, int* npos, long long* auc_num2,
                           double* ap, double* auc, void* workspace, long workspace_bytes, void* stream);

/* ---- row softmax: nn.Softmax(dim=1) closing SLICER's cluster projector (src/upstream/slicer/upstream_encoder.py:15-20);
 * fp32 [M][C]; bwd: gx = y * (gy - sum_c gy*y). */
int audiossl_softmax_rows_fwd(const float* x, float* y, int M, int C, void* stream);
int audiossl_softmax_rows_bwd(const float* y, const float* gy, float* gx, int M, int C, void* stream);

/* ---- K18 AST / MAST transformer encoder (BASELINE config 4, "AST-base 12x768"): the ViT timm builds for ASTModel,
 * extras/mast_new/mast/models/ast_work.py:70-81, 101, 183-230; optimiser extras/mast_new/mast/moco_model.py:373-379 ----
 * attn_fwd: qkv bf16 [B*S][3*H*64] (q | k | v column blocks, head h at columns h*64) -> out bf16 [B*S][H*64] =
 *           softmax(scale * q k^T) v per (clip, head), lse fp32 [B*H][S] kept for the backward.  S <= 128 runs as one
 *           tile per (clip, head); longer sequences (10 s clips: 1,212 tokens) walk 128-token blocks, B*H <= 65535.
 * attn_bwd: dout bf16 [B*S][H*64] -> dqkv bf16 [B*S][3*H*64].  `out` = what attn_fwd wrote (needed when S > 128: the
 *           multi-block backward takes D = rowsum(dout * out) from it; may be NULL for S <= 128).
 * layernorm_fwd: x fp32 [M][C] -> y bf16 (+ the same in fp32 into y32 when it is not NULL), mean / rstd fp32 [M] (C <= 1024;
 *            the MViT widths are 96 * 2^k).
 * layernorm_bwd: dres fp32 [M][C] += dx (the residual-stream gradient accumulates in place); dgamma, dbeta += .
 * gelu_fwd / gelu_bwd: exact GELU on bf16, da = dh * gelu'(a).
 * patch_unfold: x fp32 [B][F][T] -> bf16 [B*nf*nt][256], 16x16 patches, strides (fstride, tstride), row = (b, pf, pt).
 * tile_rows: out[r] = scale * src[(r / group) % period]: position embedding tiled over the batch (group 1, period N), and
 *            the backward of the mean over tokens (group N, period B, scale 1/N).
 * adamw: torch.optim.AdamW on a flat buffer; `step` = device int64 holding the 1-based step count. */
int audiossl_attn_fwd(const void* qkv, void* out, float* lse, int B, int S, int H, float scale, void* stream);
int audiossl_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int B, int S, int H,
                      float scale, void* stream);
int audiossl_layernorm_fwd(const float* x, const float* gamma, const float* beta, void* y, float* y32, float* mean, float* rstd,
                           int M, int C, float eps, void* stream);
int audiossl_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                           float* dres, float* dgamma, float* dbeta, int M, int C, void* stream);
int audiossl_gelu_fwd(const void* a, void* h, long n, void* stream);
int audiossl_gelu_bwd(const void* a, const void* dh, void* da, long n, void* stream);
int audiossl_patch_unfold(const float* x, void* out, int B, int F, int T, int fstride, int tstride, void* stream);
int audiossl_tile_rows(const float* src, float* out, long rows, int period, int group, float scale, int C, void* stream);
int audiossl_adamw(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                   float weight_decay, float grad_scale, const long long* step, void* stream);

/* ---- MViTv2 pooling attention (the encoder SS-MAST instantiates: models_msn.py:147 -> ASTModel(model_size='mvit')):
 * extras/mast_new/mast/mvit/models/attention.py:12-41 (attention_pool), :44-90 (cal_rel_pos_spatial), :93-302
 * (MultiScaleAttention), :304-393 (MultiScaleBlock).  GEMMs are audiossl_gemm, LayerNorm over the width audiossl_layernorm_*.
 * mvit_pool_fwd: one of q / k / v out of qkv bf16 [B*H*W][ldq] (column block starting at col0, head h at col0 + h*d) ->
 *           out fp32 [B][heads][Ho*Wo][d] = LayerNorm_d(depthwise 3x3 conv, stride (sh, sw), pad 1, filters w [d][3][3] shared by
 *           the heads); z / mean / rstd keep the conv output and its row statistics for the backward.  w == NULL: no pooling
 *           on this path - the head split only (Ho = H, Wo = W, no LayerNorm).  d <= 128.
 * mvit_pool_bwd: dout fp32 [B][heads][Ho*Wo][d] -> the tensor's column block of dqkv bf16 [B*H*W][ldq] (written, not
 *           accumulated); dw [d][3][3], dgamma, dbeta accumulated; dz = scratch of dout's shape.
 * mvit_attn_fwd: q [B][heads][qh*qw][d], k / v [B][heads][kh*kw][d] fp32 -> out bf16 [B*qh*qw][heads*d] =
 *           softmax(scale q k^T + q . rh[ih[query row][key row]] + q . rw[iw[query col][key col]]) v (+ q when residual: the
 *           residual pooling connection), lse fp32 [B][heads][qh*qw].  rh / rw fp32 [nrh | nrw][d] (both or neither), ih / iw
 *           int32 [qh][kh], [qw][kw] row tables (device).  d in {64, 96, 128}.
 * mvit_attn_bwd: dout bf16 [B*Lq][heads*d] -> dq fp32 (written), dk / dv fp32 and drh / drw (accumulated: zero them first).
 * tokpool_max_fwd / _bwd: MaxPool2d((kh, kw), (sh, sw), padding (kh/2, kw/2)) over the token grid of x fp32 [B][H*W][C]
 *           (the skip path of a block whose queries are pooled, attention.py:343-350); arg uint8 = tap of the maximum;
 *           bwd writes dx (gathered per input token). */
int audiossl_mvit_pool_fwd(const void* qkv, int ldq, int col0, const float* w, const float* gamma, const float* beta, float* out,
                           float* z, float* mean, float* rstd, int B, int heads, int d, int H, int W, int Ho, int Wo, int sh, int sw,
                           float eps, void* stream);
int audiossl_mvit_pool_bwd(const void* qkv, int ldq, int col0, const float* w, const float* gamma, const float* dout, const float* z,
                           const float* mean, const float* rstd, float* dz, float* dw, float* dgamma, float* dbeta, void* dqkv, int B,
                           int heads, int d, int H, int W, int Ho, int Wo, int sh, int sw, void* stream);
int audiossl_mvit_attn_fwd(const float* q, const float* k, const float* v, const float* rh, const float* rw, const int* ih,
                           const int* iw, void* out, float* lse, int B, int heads, int d, int qh, int qw, int kh, int kw, int nrh,
                           int nrw, int residual, float scale, void* stream);
int audiossl_mvit_attn_bwd(const float* q, const float* k, const float* v, const float* rh, const float* rw, const int* ih,
                           const int* iw, const void* dout, const float* lse, float* dq, float* dk, float* dv, float* drh, float* drw,
                           int B, int heads, int d, int qh, int qw, int kh, int kw, int nrh, int nrw, int residual, float scale,
                           void* stream);
int audiossl_tokpool_max_fwd(const float* x, float* y, void* arg, int B, int H, int W, int C, int kh, int kw, int sh, int sw,
                             void* stream);
int audiossl_tokpool_max_bwd(const float* dy, const void* arg, float* dx, int B, int H, int W, int C, int kh, int kw, int sh, int sw,
                             void* stream);

/* ---- LARS: extras/delores-s/multi_proc.py:4-43, on the flat parameter buffer ---------------------------------------
 * seg: n_seg x {int64 offset, int64 numel, int32 flags (bit0 weight decay, bit1 trust ratio), int32 pad} (device);
 * lr: per-segment learning rate (device); norms: 2*n_seg doubles of scratch. */
int audiossl_lars_step(float* p, const float* g, float* mu, const void* seg, int n_seg, const float* lr, float weight_decay,
                       float momentum, float eta, float grad_scale, double* norms, void* stream);
/* apex LARC around torch.optim.SGD (`extras/decar-v2/main.py:92-97, 111`: SGD(momentum 0.9, wd 1e-6) wrapped in
 * LARC(trust_coefficient 0.001, clip False)): per tensor alr = tc |p| / (|g| + wd |p| + eps) when both norms are non-zero,
 * g' = (g + wd p) alr, else g' = g; then buf = m buf + g', p -= lr buf.  seg as lars_step; flags & 4 = no gradient this step
 * (the reference sets p.grad = None for frozen prototypes: the tensor and its momentum are left untouched). */
int audiossl_larc_step(float* p, const float* g, float* mu, const void* seg, int n_seg, float lr, float weight_decay,
                       float momentum, float trust_coefficient, float eps, int clip, float grad_scale, double* norms,
                       void* stream);

/* ---- Linear evaluation on cached embeddings: a grid of H heads trained together (csrc/probe.hip, src/evaluation/probe.py).
 * The heads are one fp32 matrix W [H * Cp][Dp], Cp = C rounded up to a multiple of 8: head h owns rows [h Cp, h Cp + C), its
 * pad rows are zero and never move (their gradient is exactly zero).  Dp = D + 8: the batch carries 1.0 in column D, so the
 * bias is column D of W and is decayed like the weights, as torch.optim.AdamW(linear.parameters(), weight_decay) does.  The two
 * GEMMs of a step are audiossl_gemm with dtype 0: logits [B][H Cp] = Xb W^T and dW = G^T Xb (both transposes set: any B).
 * probe_batch: out[r][0:D] = (X[idx[r]][:] - mean[:]) * rstd[:] in fp32, subtract then multiply, each rounded once (equal to
 *   numpy fp32 bit for bit); mean and rstd NULL together = a plain gather.  out[r][D] = 1, out[r][D+1 : ldo] = 0.  X [N][D]
 *   row-major, idx int32 [B] on the device, rows may repeat.  An index outside [0, N) is never dereferenced: all ldo columns of
 *   its row are NaN.  D % 8 == 0, 8 <= D <= 4096, ldo >= D + 8, ldo % 4 == 0.
 * probe_ce: for every row r and head h, over columns [h Cp, h Cp + C) of logits [B][ld]: stable soft-max cross-entropy against
 *   label[r] (int64).  loss_sum[h] (fp64) += the sum of the row losses, correct[h] (int64) += the rows whose first arg-max (ties
 *   to the lowest class, as torch.argmax) equals the label; both have one writer that sums in a fixed order, no atomics: two
 *   launches on the same input agree bit for bit.  dlogits[r][h Cp + c] = gscale (p - 1[c == label]) for c < C and exactly 0
 *   for the pad columns; columns at and beyond H Cp are not touched.  dlogits NULL = evaluation, the same loss_sum and correct
 *   bit for bit.  A label outside [0, C) is never used as an index: it adds NaN to every loss_sum[h], and that row's class
 *   columns of dlogits are NaN (pad columns still 0).  2 <= C <= 4096, Cp >= C, Cp % 4 == 0, H >= 1, ld >= H Cp, ld % 4 == 0.
 * probe_adamw: torch.optim.AdamW with one parameter group per head: segment h = [h seg, (h + 1) seg) of the flat W / dW / m / v
 *   uses lr[h] * lr_scale and wd[h] (device fp32 [H]); `step` = device int64 holding the 1-based count, as in audiossl_adamw,
 *   whose per-element arithmetic this is (csrc/adamw.h); the betas are fp64, and 1 - beta and the two bias corrections are
 *   formed in fp64 before they are rounded, as torch forms them on the host.  A head with lr = 0 and wd = 0 keeps W bit-unchanged.  seg % 4 == 0.
 * None of the three synchronises with the host; all validate before any launch. */
int audiossl_probe_batch(const float* X, long N, int D, const int* idx, int B, const float* mean, const float* rstd, float* out,
                         long ldo, void* stream);
int audiossl_probe_ce(const float* logits, long ld, const long long* label, int B, int H, int C, int Cp, float gscale,
                      double* loss_sum, long long* correct, float* dlogits, void* stream);
int audiossl_probe_adamw(float* W, const float* dW, float* m, float* v, int H, long seg, const float* lr, const float* wd,
                         float lr_scale, double beta1, double beta2, float eps, const long long* step, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AUDIOSSL_HIP_H */
