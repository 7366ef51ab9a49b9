// qgd_fused_caps.hpp -- the caps of a cell block of the fused kernels (qgd_setup.hpp FusedBlocks), seen by the host code that cuts the
// blocks (qgd_setup.cpp, qgd_capi.cpp) and by the kernels whose register and LDS budgets are sized for them (qgd_kernels.hip
// fusedFaceCellKernel, qgd_qhd.hip qhdFusedAdvanceKernel: their static_asserts).
#pragma once
#include <cstdint>

namespace qgd {

// own cells; own + across-a-face cells; vertices; internal faces; all staged cells (+ the edge / corner cells around the vertices)
constexpr int32_t kFusedCells = 128, kFusedCapC = 320, kFusedCapV = 256, kFusedCapF = 512, kFusedCapTot = 384;

}  // namespace qgd
