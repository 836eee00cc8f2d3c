// DTU accuracy / completeness evaluation of a fused point cloud (the reference's DTU-MATLAB folder:
// reducePts_haa.m, MaxDistCP.m, PointCompareMain.m), as uniform-grid searches:
//
//   grid index   per point a 64-bit key of its cell floor((p - origin) / cell) (fp64), 21 bits per axis,
//                z in the low bits; the caller sorts the keys; tmvs_dtu_grid_table turns the sorted keys
//                into the table of unique keys and run starts; the sorted points are float4 records
//                (x, y, z, one int32 of payload). The z cells of one (x, y) column that exist are
//                neighbours in the table, so one binary search finds a whole z range of a column.
//   thinning     reducePts_haa.m:17-31 is the lexicographically-first maximal independent set of the
//                "within dst" graph under its visiting order. One launch per round over point states:
//                an undecided point is removed when a neighbour of smaller rank is kept, kept when every
//                neighbour of smaller rank is removed. States are read from the previous round's buffer
//                and written to the next, so the launch boundary is the only ordering.
//   nearest      MaxDistCP.m:25-36 restricted to distances < max_dist <= block: expanding rings of cells
//                round the from-point's cell, stopped when the ring's inner distance reaches the best
//                found. A pass refines d2 in place, so a fine grid (rings 0-1) settles the dense part and
//                a coarse grid finishes the outliers through few, mostly empty, cells.
//
// Every comparison is made in fp64 on squared distances, in the fixed unfused order
// dx = (double)a.x - (double)b.x, d2 = (dx*dx + dy*dy) + dz*dz (the build passes -ffp-contract=off).
#include <math.h>

#include "common.h"

namespace tmvs {

namespace dtu {
constexpr long long HALF = 1LL << 20;  // cell indices live in [-HALF, HALF)
constexpr int UNDECIDED = TMVS_DTU_UNDECIDED, KEPT = TMVS_DTU_KEPT, REMOVED = TMVS_DTU_REMOVED;

struct Grid {
  double ox, oy, oz, cell;
  const long long* ukeys;  // [ncells] ascending
  const int* ustart;       // [ncells + 1]
  int ncells;
  int npts;
};

// floor((p - o) / cell), clamped into the index range (a NaN lands on -HALF). Clamping is monotone and
// moves no two indices further apart, so points within one cell edge stay in neighbouring cells.
__device__ __forceinline__ long long cell_index(double p, double o, double cell) {
  const double q = floor((p - o) / cell);
  return (long long)fmin(fmax(q, (double)-HALF), (double)(HALF - 1));
}
__device__ __forceinline__ long long pack_key(long long ix, long long iy, long long iz) {
  return ((ix + HALF) << 42) | ((iy + HALF) << 21) | (iz + HALF);
}
__device__ __forceinline__ double dist2(double ax, double ay, double az, const float4& b) {
  const double dx = ax - (double)b.x, dy = ay - (double)b.y, dz = az - (double)b.z;
  return (dx * dx + dy * dy) + dz * dz;
}

// Calls f(j) for every sorted point j in the cells (ix, iy, z0..z1); false from f stops the walk.
template <typename F>
__device__ __forceinline__ bool scan_column(const Grid& g, long long ix, long long iy, long long z0, long long z1,
                                            F f) {
  if (ix < -HALF || ix >= HALF || iy < -HALF || iy >= HALF) return true;
  z0 = z0 < -HALF ? -HALF : z0;
  z1 = z1 >= HALF ? HALF - 1 : z1;
  if (z0 > z1) return true;
  const long long klo = pack_key(ix, iy, z0), khi = pack_key(ix, iy, z1);
  int lo = 0, hi = g.ncells;  // first cell with key >= klo
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (g.ukeys[mid] < klo) lo = mid + 1;
    else hi = mid;
  }
  int c = lo;
  while (c < g.ncells && g.ukeys[c] <= khi) ++c;
  if (c == lo) return true;
  int j = g.ustart[lo], je = g.ustart[c];
  j = j < 0 ? 0 : j;
  je = je > g.npts ? g.npts : je;
  for (; j < je; ++j)
    if (!f(j)) return false;
  return true;
}
}  // namespace dtu

__global__ __launch_bounds__(256) void dtu_cell_keys_kernel(const float* __restrict__ xyz, long n, double ox, double oy,
                                                            double oz, double cell, long long* __restrict__ keys) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  keys[i] = dtu::pack_key(dtu::cell_index((double)xyz[3 * i], ox, cell), dtu::cell_index((double)xyz[3 * i + 1], oy, cell),
                          dtu::cell_index((double)xyz[3 * i + 2], oz, cell));
}

__global__ __launch_bounds__(256) void dtu_gather_kernel(const float* __restrict__ xyz, const long long* __restrict__ order,
                                                         const int* __restrict__ payload, long n,
                                                         float4* __restrict__ pts) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long o = order[i];
  float4 p = make_float4(NAN, NAN, NAN, __int_as_float(-1));  // an index outside [0, n) is never read
  if (o >= 0 && o < n) p = make_float4(xyz[3 * o], xyz[3 * o + 1], xyz[3 * o + 2], __int_as_float(payload ? payload[o] : (int)o));
  pts[i] = p;
}

__global__ __launch_bounds__(256) void dtu_grid_table_kernel(const long long* __restrict__ keys,
                                                             const long long* __restrict__ rank, long n, long ncells,
                                                             long long* __restrict__ ukeys, int* __restrict__ ustart) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long k = keys[i];
  if (i == 0 || keys[i - 1] != k) {
    const long long r = rank[i] - 1;
    if (r >= 0 && r < ncells) {
      ukeys[r] = k;
      ustart[r] = (int)i;
    }
  }
  if (i == n - 1) ustart[ncells] = (int)n;
}

__global__ __launch_bounds__(256) void dtu_thin_round_kernel(const float4* __restrict__ pts, dtu::Grid g, double r2,
                                                             const unsigned char* __restrict__ state_in,
                                                             unsigned char* __restrict__ state_out,
                                                             int* __restrict__ undecided) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= g.npts) return;
  int s = state_in[i];
  if (s == dtu::UNDECIDED) {
    const float4 p = pts[i];
    const int rank = __float_as_int(p.w);
    const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
    const long long ix = dtu::cell_index(px, g.ox, g.cell), iy = dtu::cell_index(py, g.oy, g.cell),
                    iz = dtu::cell_index(pz, g.oz, g.cell);
    bool kept_nb = false, open_nb = false;
    for (int dx = -1; dx <= 1 && !kept_nb; ++dx)
      for (int dy = -1; dy <= 1 && !kept_nb; ++dy)
        dtu::scan_column(g, ix + dx, iy + dy, iz - 1, iz + 1, [&](int j) {
          const float4 q = pts[j];
          if (__float_as_int(q.w) >= rank) return true;  // itself and every later visit
          if (dtu::dist2(px, py, pz, q) <= r2) {
            const int sj = state_in[j];
            if (sj == dtu::KEPT) {
              kept_nb = true;
              return false;
            }
            if (sj == dtu::UNDECIDED) open_nb = true;
          }
          return true;
        });
    s = kept_nb ? dtu::REMOVED : (open_nb ? dtu::UNDECIDED : dtu::KEPT);
    if (s == dtu::UNDECIDED) atomicAdd(undecided, 1);
  }
  state_out[i] = (unsigned char)s;
}

__global__ __launch_bounds__(256) void dtu_nearest_pass_kernel(const float4* __restrict__ from, int nfrom,
                                                               const float4* __restrict__ to, dtu::Grid g, int max_ring,
                                                               double skip_below, double lox, double loy, double loz,
                                                               double hix, double hiy, double hiz,
                                                               double* __restrict__ d2) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nfrom) return;
  const float4 p = from[i];
  const int idx = __float_as_int(p.w);
  if (idx < 0 || idx >= nfrom) return;
  const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
  // MaxDistCP.m:16-17: only from-points inside a block are given a distance (a NaN is in none)
  if (!(px >= lox && px < hix && py >= loy && py < hiy && pz >= loz && pz < hiz)) return;
  double best = d2[idx];
  if (!(best > skip_below)) return;
  const long long ix = dtu::cell_index(px, g.ox, g.cell), iy = dtu::cell_index(py, g.oy, g.cell),
                  iz = dtu::cell_index(pz, g.oz, g.cell);
  // a point of ring r is at least (r - 1) cell edges away; the slack covers the rounding of cell_index
  const double slack = g.cell * 1e-6;
  auto visit = [&](int j) {
    const double v = dtu::dist2(px, py, pz, to[j]);
    if (v < best) best = v;
    return true;
  };
  for (int r = 0; r <= max_ring; ++r) {
    if (r >= 2) {
      const double inner = (double)(r - 1) * g.cell - slack;
      if (inner * inner >= best) break;
    }
    for (int dx = -r; dx <= r; ++dx)
      for (int dy = -r; dy <= r; ++dy) {
        const int m = (dx < 0 ? -dx : dx) > (dy < 0 ? -dy : dy) ? (dx < 0 ? -dx : dx) : (dy < 0 ? -dy : dy);
        if (m == r) {
          dtu::scan_column(g, ix + dx, iy + dy, iz - r, iz + r, visit);
        } else {  // the ring's floor and ceiling above an inner column
          dtu::scan_column(g, ix + dx, iy + dy, iz - r, iz - r, visit);
          dtu::scan_column(g, ix + dx, iy + dy, iz + r, iz + r, visit);
        }
      }
  }
  d2[idx] = best;
}

// PointCompareMain.m:37-45: Qv = round((Q - BB1) / Res + 1) (half away from zero), inside 1..size and set
__global__ __launch_bounds__(256) void dtu_in_mask_kernel(const float* __restrict__ xyz, long n,
                                                          const unsigned char* __restrict__ mask, int X, int Y, int Z,
                                                          double bx, double by, double bz, double res,
                                                          unsigned char* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double qx = round(((double)xyz[3 * i] - bx) / res + 1.0);
  const double qy = round(((double)xyz[3 * i + 1] - by) / res + 1.0);
  const double qz = round(((double)xyz[3 * i + 2] - bz) / res + 1.0);
  unsigned char r = 0;
  if (qx > 0.0 && qx <= (double)X && qy > 0.0 && qy <= (double)Y && qz > 0.0 && qz <= (double)Z)
    r = mask[((size_t)((long)qx - 1) * Y + (size_t)((long)qy - 1)) * Z + (size_t)((long)qz - 1)] ? 1 : 0;
  out[i] = r;
}

// PointCompareMain.m:57: P' * [Q; 1] > 0
__global__ __launch_bounds__(256) void dtu_above_plane_kernel(const float* __restrict__ xyz, long n, double p0, double p1,
                                                              double p2, double p3, unsigned char* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double v = ((p0 * (double)xyz[3 * i] + p1 * (double)xyz[3 * i + 1]) + p2 * (double)xyz[3 * i + 2]) + p3;
  out[i] = v > 0.0 ? 1 : 0;
}

}  // namespace tmvs

using namespace tmvs;

namespace {
constexpr long kMaxPoints = 2147483647L - 256;  // int32 positions and 1-D grids of 256-thread blocks
inline bool good_n(long n) { return n > 0; }
inline bool good_grid(const double* g) {
  return g && isfinite(g[0]) && isfinite(g[1]) && isfinite(g[2]) && isfinite(g[3]) && g[3] > 0.0;
}
inline unsigned blocks(long n) { return (unsigned)((n + 255) / 256); }
inline dtu::Grid make_grid(const double* g, const void* table, long n_cells, long n_points) {
  dtu::Grid r;
  r.ox = g[0], r.oy = g[1], r.oz = g[2], r.cell = g[3];
  r.ukeys = (const long long*)table;
  r.ustart = (const int*)((const char*)table + 8 * (size_t)n_cells);
  r.ncells = (int)n_cells;
  r.npts = (int)n_points;
  return r;
}
}  // namespace

extern "C" int tmvs_dtu_cell_keys(const float* xyz, long n, const double* grid, long long* keys, void* stream) {
  if (!xyz || !keys || !good_grid(grid) || !good_n(n)) return TMVS_ERR_ARG;
  if (n > kMaxPoints) return TMVS_ERR_SHAPE;
  hipLaunchKernelGGL(dtu_cell_keys_kernel, dim3(blocks(n)), dim3(256), 0, (hipStream_t)stream, xyz, n, grid[0], grid[1],
                     grid[2], grid[3], keys);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

extern "C" int tmvs_dtu_gather_points(const float* xyz, const long long* order, const int* payload, long n,
                                      float* points4, void* stream) {
  if (!xyz || !order || !points4 || !good_n(n)) return TMVS_ERR_ARG;
  if (n > kMaxPoints) return TMVS_ERR_SHAPE;
  if ((uintptr_t)points4 % 16) return TMVS_ERR_ARG;
  hipLaunchKernelGGL(dtu_gather_kernel, dim3(blocks(n)), dim3(256), 0, (hipStream_t)stream, xyz, order, payload, n,
                     (float4*)points4);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

extern "C" size_t tmvs_dtu_grid_table_bytes(long n_cells) {
  if (n_cells <= 0 || n_cells > kMaxPoints) return 0;
  return ((size_t)n_cells * 8 + ((size_t)n_cells + 1) * 4 + 15) / 16 * 16;
}

extern "C" int tmvs_dtu_grid_table(const long long* sorted_keys, const long long* head_rank, long n, long n_cells,
                                   void* table, size_t table_bytes, void* stream) {
  if (!sorted_keys || !head_rank || !table || !good_n(n) || n_cells <= 0 || n_cells > n) return TMVS_ERR_ARG;
  if (n > kMaxPoints) return TMVS_ERR_SHAPE;
  if ((uintptr_t)table % 8 || table_bytes < tmvs_dtu_grid_table_bytes(n_cells)) return TMVS_ERR_ARG;
  hipLaunchKernelGGL(dtu_grid_table_kernel, dim3(blocks(n)), dim3(256), 0, (hipStream_t)stream, sorted_keys, head_rank,
                     n, n_cells, (long long*)table, (int*)((char*)table + 8 * (size_t)n_cells));
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

extern "C" int tmvs_dtu_thin_round(const float* points4, long n, const void* table, long n_cells, const double* grid,
                                   double radius, const unsigned char* state_in, unsigned char* state_out,
                                   int* undecided, void* stream) {
  if (!points4 || !table || !state_in || !state_out || !undecided || state_in == state_out) return TMVS_ERR_ARG;
  if (!good_grid(grid) || !good_n(n) || n_cells <= 0 || n_cells > n) return TMVS_ERR_ARG;
  // the 3x3x3 neighbourhood holds every point within the radius only when a cell is wider than it
  if (!(radius > 0.0) || !(radius < grid[3])) return TMVS_ERR_ARG;
  if (n > kMaxPoints) return TMVS_ERR_SHAPE;
  if ((uintptr_t)points4 % 16 || (uintptr_t)table % 8) return TMVS_ERR_ARG;
  hipLaunchKernelGGL(dtu_thin_round_kernel, dim3(blocks(n)), dim3(256), 0, (hipStream_t)stream, (const float4*)points4,
                     make_grid(grid, table, n_cells, n), radius * radius, state_in, state_out, undecided);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

extern "C" int tmvs_dtu_nearest_pass(const float* from4, long n_from, const float* to4, long n_to, const void* table,
                                     long n_cells, const double* grid, const double* bb, double max_dist, double block,
                                     int max_ring, double skip_below, double* d2, void* stream) {
  if (!from4 || !to4 || !table || !bb || !d2 || !good_grid(grid)) return TMVS_ERR_ARG;
  if (!good_n(n_from) || !good_n(n_to) || n_cells <= 0 || n_cells > n_to || max_ring < 0) return TMVS_ERR_ARG;
  if (!(max_dist > 0.0) || !(block > 0.0) || !(max_dist <= block) || !isfinite(block)) return TMVS_ERR_ARG;
  if (n_from > kMaxPoints || n_to > kMaxPoints) return TMVS_ERR_SHAPE;
  if ((uintptr_t)from4 % 16 || (uintptr_t)to4 % 16 || (uintptr_t)table % 8) return TMVS_ERR_ARG;
  double hi[3];
  for (int a = 0; a < 3; ++a) {
    if (!isfinite(bb[a]) || !isfinite(bb[3 + a])) return TMVS_ERR_ARG;
    hi[a] = bb[a] + (floor((bb[3 + a] - bb[a]) / block) + 1.0) * block;  // MaxDistCP.m:5,12-13
  }
  // no ring further out than max_dist can hold a nearer point
  const double far = ceil(max_dist / grid[3]) + 2.0;
  if ((double)max_ring > far) max_ring = (int)far;
  if (max_ring > TMVS_DTU_MAX_RING) return TMVS_ERR_SHAPE;  // a ring costs (2r + 1)^2 column searches
  hipLaunchKernelGGL(dtu_nearest_pass_kernel, dim3(blocks(n_from)), dim3(256), 0, (hipStream_t)stream,
                     (const float4*)from4, (int)n_from, (const float4*)to4, make_grid(grid, table, n_cells, n_to),
                     max_ring, skip_below, bb[0], bb[1], bb[2], hi[0], hi[1], hi[2], d2);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

extern "C" int tmvs_dtu_in_mask(const float* xyz, long n, const unsigned char* mask, int size_x, int size_y, int size_z,
                                const double* bb_low, double res, unsigned char* out, void* stream) {
  if (!xyz || !mask || !bb_low || !out || !good_n(n) || size_x <= 0 || size_y <= 0 || size_z <= 0) return TMVS_ERR_ARG;
  if (!(res > 0.0) || !isfinite(res) || !isfinite(bb_low[0]) || !isfinite(bb_low[1]) || !isfinite(bb_low[2]))
    return TMVS_ERR_ARG;
  if (n > kMaxPoints) return TMVS_ERR_SHAPE;
  hipLaunchKernelGGL(dtu_in_mask_kernel, dim3(blocks(n)), dim3(256), 0, (hipStream_t)stream, xyz, n, mask, size_x, size_y,
                     size_z, bb_low[0], bb_low[1], bb_low[2], res, out);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

extern "C" int tmvs_dtu_above_plane(const float* xyz, long n, const double* plane, unsigned char* out, void* stream) {
  if (!xyz || !plane || !out || !good_n(n)) return TMVS_ERR_ARG;
  if (n > kMaxPoints) return TMVS_ERR_SHAPE;
  hipLaunchKernelGGL(dtu_above_plane_kernel, dim3(blocks(n)), dim3(256), 0, (hipStream_t)stream, xyz, n, plane[0],
                     plane[1], plane[2], plane[3], out);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}
