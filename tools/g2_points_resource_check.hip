// The decode / validate kernels alone, for `hipcc --cuda-device-only -c -Rpass-analysis=kernel-resource-usage` (tests/test_g2_points_cpu.py reads the
// remarks: no kernel may use scratch memory).  Compiled with -DMSM_HIP_TEST_HOOKS so that the hook kernel is there too.
#include "../gpu-acceleration_amd/csrc/msm_kernels_g2_points.hpp"
template __global__ void msmk::k_g2_decompress<false>(const uint32_t*, uint32_t, uint32_t*, uint8_t*, uint32_t*);
template __global__ void msmk::k_g2_decompress<true>(const uint32_t*, uint32_t, uint32_t*, uint8_t*, uint32_t*);
