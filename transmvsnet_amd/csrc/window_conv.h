// What FeatureNet's three persistent "window" kernels (featurenet.hip: dcn_window_kernel,
// conv3x3_window_kernel; conv2d.hip: conv2d_bn_relu_kernel) have in one copy: the layout of the LDS window
// and the persistent grid of their launchers. Each kernel's unit walk, copy loops, tap loop and epilogue are
// its own (profiles/featurenet_scaffold_resources.md).
#pragma once
#include "common.h"

#include <algorithm>

namespace tmvs {
namespace wconv {

// ---- window: WR x WC pixels of G 16-byte chunks (4 channels each), copied by NT threads.
// Slot of chunk c of window pixel P: the chunk index is XORed with bits of P, so that both the copy
// (consecutive lanes = consecutive chunks) and the B-layout reads (16 pixels per lane group) are
// bank-conflict-free.
template <int G_, int SH_, int WR_, int WC_, int NT_>
struct Window {
  static constexpr int G = G_, SH = SH_, WR = WR_, WC = WC_, NT = NT_;
  static constexpr int WIN4 = WR * WC * G;            // window float4s
  static constexpr int STAGE = (WIN4 + NT - 1) / NT;  // float4 per thread per window copy
  static __device__ __forceinline__ int slot(int P, int c) { return G == 1 ? P : P * G + (c ^ ((P >> SH) & (G - 1))); }
};

// ---- host: the persistent grid of a window kernel: one workgroup per CU slot its LDS / VGPR footprint
// allows, at most one per unit; the slot count is cached per kernel instance. 0: no device.
template <auto KERNEL>
int persistent_blocks(int threads, long long nunits) {
  static int grid = 0;
  if (!grid) {
    int dev = 0, ncu = 0, occ = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, KERNEL, threads, 0);
    grid = std::max(1, ncu * std::max(occ, 1));
  }
  return (int)std::min<long long>(grid, nunits);
}

}  // namespace wconv
}  // namespace tmvs
