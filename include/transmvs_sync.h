/* transmvs_sync.h -- the C-ABI of BatchNorm statistics synchronised across ranks (SyncBN).
 *
 * A second header next to transmvs.h, with its conventions (extern "C", stateless, no allocation and no host
 * synchronisation inside a call, DEVICE pointers, scratch memory passed in, `stream` a hipStream_t or NULL, an int
 * status). transmvsnet_amd/sync_bn.py binds and drives these entries; DESIGN.md "Synchronised BatchNorm" has the
 * protocol. The library does no communication: it offers the train-mode BatchNorm passes of transmvs.h cut where
 * their reductions have to cross ranks.
 *
 *   - Only fp64 raw sums cross ranks: what the fixed-order sum of the block partials gives, before any finalize.
 *   - Each rank writes its sums into slot `rank` of a zero-filled [world][K] buffer; one all-reduce(SUM) of that
 *     buffer acts as a gather (adding zeros is exact); tmvs_rank_sum adds the slots in rank order. The combine
 *     is therefore bit-identical on every rank and independent of the backend's reduction algorithm.
 *   - The entries that consume sums take `n_total`, the number of elements behind them (all ranks'), and do not
 *     assume equal counts per rank. Fed a rank's own sums with n_total = its own count they are the fused
 *     entries of transmvs.h bit for bit (the same kernels).
 *   - Parameter gradients (dgamma / dbeta, PixelwiseNet's dpwp) stay this rank's local sums: the gradient
 *     all-reduce averages them afterwards, as DistributedDataParallel does after torch.nn.SyncBatchNorm.
 *
 * Errors as in transmvs.h: a null pointer, a non-positive extent, world <= 0, an n_total below the rank's own
 * count or a workspace too small TMVS_ERR_ARG; a BatchNorm channel count that does not divide 256
 * TMVS_ERR_SHAPE; all before anything is enqueued.                                                          */
#ifndef TRANSMVS_SYNC_H_
#define TRANSMVS_SYNC_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* out[i] = slots[0][i] + slots[1][i] + ... + slots[world-1][i], i < count, fp64, added in that order
 * (world == 1: a copy). slots [world][count]; out must not alias it.                                       */
int tmvs_rank_sum(const double* slots, int world, long count, double* out, void* stream);

/* ---- grouped BatchNorm + ReLU (tmvs_bn_stats_grouped / tmvs_bn_relu_backward_grouped, split) ------------
 * z, dy, dz [groups][nvox][channels]; mean, var [groups][channels]; gamma, beta, dgamma, dbeta [channels];
 * sums fp64 [groups][2][channels]. workspace: tmvs_bn_train_workspace_grouped(groups, nvox, channels) bytes.
 * The ungrouped BatchNorm is groups = 1; the forward apply is tmvs_bn_relu_train[_grouped], unchanged.
 *
 * tmvs_bn_moments_grouped:            sums = (sum z, sum z^2) per group and channel, no finalize.
 * tmvs_bn_stats_from_sums:            mean = s / n_total, var = max(s2 / n_total - mean^2, 0) (biased), fp32.
 * tmvs_bn_relu_backward_sums_grouped: sums = (sum g, sum g * xhat), g = dy where the BatchNorm output is
 *     positive; dbeta / dgamma from these local sums, per group in fp32, then added over the groups in order.
 * tmvs_bn_relu_backward_apply_grouped: dz = gamma * rstd * ((g - S_g / n_total) - xhat * S_gx / n_total)
 *     with global_sums = (S_g, S_gx) over all ranks. n_total >= nvox.                                       */
int tmvs_bn_moments_grouped(const float* z, int groups, long nvox, int channels, void* workspace,
                            size_t workspace_bytes, double* sums, void* stream);
int tmvs_bn_stats_from_sums(const double* sums, int groups, int channels, long n_total, float* mean, float* var,
                            void* stream);
int tmvs_bn_relu_backward_sums_grouped(const float* dy, const float* z, int groups, long nvox, int channels,
                                       const float* mean, const float* var, const float* gamma, const float* beta,
                                       float eps, void* workspace, size_t workspace_bytes, double* sums,
                                       float* dgamma, float* dbeta, void* stream);
int tmvs_bn_relu_backward_apply_grouped(const float* dy, const float* z, int groups, long nvox, int channels,
                                        const float* mean, const float* var, const float* gamma, const float* beta,
                                        float eps, const double* global_sums, long n_total, float* dz, void* stream);

/* ---- PixelwiseNet in train mode (tmvs_pixelwise_train_forward_batched / _backward_batched, staged) ------
 * Tensors as there: sims, dsims [batch][n_views][ndepth][height][width], pwp [201], stats [n_views][48],
 * view_w, dview_w, dstar [batch][n_views][height][width]. Each entry runs one stage for all views, so one
 * collective per stage serves them all. workspace: tmvs_pixelwise_train_workspace() bytes. n_total: the
 * elements of one view on all ranks, at least batch * ndepth * height * width.
 *
 * forward:  _forward_sums    -> s_sums [n_views][2]   = (sum s, sum s^2)
 *           _forward_z1      <- global s_sums; writes the layer-0 statistics into stats
 *                            -> z1_sums [n_views][16] = (sum z1[8], sum z1^2[8])
 *           _forward_weights <- global z1_sums; writes the layer-1 statistics, view_w and dstar
 * backward: _backward_s1     -> s1 [n_views][25]      (tmvs_pixelwise_train_backward's pass 1)
 *           _backward_s2     <- global s1             -> s2 [n_views][160] (pass 2)
 *           _backward_apply  <- global s1, global s2: adds the PixelwiseNet path into dsims (pass 3), and the
 *                            parameter gradients of this rank's local_s1 / local_s2 / pass-3 sums into dpwp
 *                            (views in order). Only the BatchNorm sums of s1 (first 16) and s2 (first 32) are
 *                            read from the global buffers.                                                  */
int tmvs_pw_sync_forward_sums(const float* sims, int batch, int n_views, int ndepth, int height, int width,
                              void* workspace, size_t workspace_bytes, double* s_sums, void* stream);
int tmvs_pw_sync_forward_z1(const float* sims, int batch, int n_views, int ndepth, int height, int width,
                            const float* pwp, const double* s_sums, long n_total, void* workspace,
                            size_t workspace_bytes, float* stats, double* z1_sums, void* stream);
int tmvs_pw_sync_forward_weights(const float* sims, int batch, int n_views, int ndepth, int height, int width,
                                 const float* pwp, const double* z1_sums, long n_total, float* stats, float* view_w,
                                 int* dstar, void* stream);
int tmvs_pw_sync_backward_s1(const float* sims, int batch, int n_views, int ndepth, int height, int width,
                             const float* pwp, const float* stats, const float* view_w, const int* dstar,
                             const float* dview_w, void* workspace, size_t workspace_bytes, double* s1, void* stream);
int tmvs_pw_sync_backward_s2(const float* sims, int batch, int n_views, int ndepth, int height, int width,
                             const float* pwp, const float* stats, const float* view_w, const int* dstar,
                             const float* dview_w, const double* global_s1, long n_total, void* workspace,
                             size_t workspace_bytes, double* s2, void* stream);
int tmvs_pw_sync_backward_apply(const float* sims, int batch, int n_views, int ndepth, int height, int width,
                                const float* pwp, const float* stats, const float* view_w, const int* dstar,
                                const float* dview_w, const double* global_s1, const double* global_s2, long n_total,
                                const double* local_s1, const double* local_s2, void* workspace,
                                size_t workspace_bytes, float* dsims, float* dpwp, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TRANSMVS_SYNC_H_ */
