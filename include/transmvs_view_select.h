/* transmvs_view_select.h -- the C-ABI of view selection for a COLMAP sparse model (MVSNet's view-selection
 * score, Yao et al. 2018, section 4.1): which views see which 3-D points, the depth of every observation, and
 * the score of every pair of views.
 *
 * A third header next to transmvs.h and transmvs_sync.h, with their conventions (extern "C", stateless, no
 * allocation and no host synchronisation inside a call, DEVICE pointers unless marked, `stream` a hipStream_t or
 * NULL, an int status). transmvsnet_amd/view_select.py binds these entries, transmvsnet_amd/colmap_scene.py
 * drives them; DESIGN.md "COLMAP scene import" has the algorithm. They are additions, so TMVS_ABI_VERSION stays.
 *
 * Sizes: V views, P points, M observations = (view, point) int32 pairs, in any order, duplicates allowed.
 * W = (P + 63) / 64. All arithmetic is fp64 and unfused (the build passes -ffp-contract=off).
 * V < 2, P < 1, P >= 2^31 - 64, M < 1, M >= 2^31 - 256 are TMVS_ERR_SHAPE, as is a bit matrix above
 * TMVS_VS_MAX_BITS_BYTES; a null pointer or a misaligned `bits` TMVS_ERR_ARG; all before anything is enqueued.
 *
 * `errors` is one device int32, zeroed by the caller. An observation whose view is outside [0, V) or whose
 * point is outside [0, P) is never used as an index: nothing is written for it by tmvs_vs_set_bits, NaN by
 * tmvs_vs_obs_depth, and *errors is increased by one.
 *
 * tmvs_vs_set_bits: bits [V][W] uint64 (8-byte aligned, zeroed by the caller): bit p % 64 of word p / 64 of
 *   row v is set for every observation (v, p), by 64-bit atomic OR, which is idempotent: duplicates and
 *   the order of the observations do not show in the result.
 * tmvs_vs_obs_depth: z[m] = ((r0 x + r1 y) + r2 z) + tz[v] for observation m = (v, p), with (r0, r1, r2) =
 *   R3[v] (the third row of the view's rotation, R3 [V][3]), tz [V] and (x, y, z) = xyz[p] (xyz [P][3]).
 * tmvs_vs_pair_scores: for every pair of views i < j, over the points p < P whose bit is set in both rows
 *   (bits at positions >= P of a row's last word are ignored whatever they hold):
 *     counts[i][j] = counts[j][i] = their number (int32),
 *     scores[i][j] = scores[j][i] = the sum of exp(-(theta - theta0)^2 / (2 sigma^2)) (fp64), where
 *       a = C_i - X, b = C_j - X (centres [V][3], X = xyz[p]), c = a x b,
 *       theta = atan2(sqrt((cx cx + cy cy) + cz cz), (ax bx + ay by) + az bz) * (180 / pi)   (degrees),
 *       sigma = sigma1 when theta <= theta0, else sigma2.
 *   The diagonals are written as 0. scores and counts are [V][V]. theta0, sigma1, sigma2 must be finite and
 *   the sigmas positive (TMVS_ERR_ARG).
 *   The order of summation is fixed, so the scores repeat bit for bit: a pair is summed by one 256-thread
 *   block; thread t owns the word couples q = t, t + 256, t + 512, ... (couple q = words 2q and 2q + 1 of the
 *   rows) and adds the terms of its points in ascending point order into one fp64 partial, starting from 0;
 *   the 256 partials are added inside each wave of 64 by the xor butterfly x += x[lane ^ off], off = 32, 16,
 *   8, 4, 2, 1, and the four wave sums as (w0 + w1) + (w2 + w3). There are no floating-point atomics. */
#ifndef TRANSMVS_VIEW_SELECT_H_
#define TRANSMVS_VIEW_SELECT_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMVS_VS_MAX_BITS_BYTES 1073741824 /* 1 GiB: V * W * 8 above it is refused, nothing is paged */
#define TMVS_VS_MAX_BLOCKS 2048           /* the grid cap of tmvs_vs_pair_scores: a block walks pairs b, b + grid, ... */

int tmvs_vs_set_bits(const int* obs_view, const int* obs_point, long n_obs, int n_views, long n_points,
                     unsigned long long* bits, int* errors, void* stream);
int tmvs_vs_obs_depth(const int* obs_view, const int* obs_point, long n_obs, int n_views, long n_points,
                      const double* r3, const double* tz, const double* xyz, double* z, int* errors, void* stream);
int tmvs_vs_pair_scores(const unsigned long long* bits, int n_views, long n_points, const double* centres,
                        const double* xyz, double theta0, double sigma1, double sigma2, double* scores, int* counts,
                        void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TRANSMVS_VIEW_SELECT_H_ */
