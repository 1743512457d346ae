/* Host-side HIP helpers shared by the aligner seam (gpu_align.cpp) and the
 * device-resident batch driver (gpu_batch_resident.cpp). Internal: C++ only,
 * included after <hip/hip_runtime.h>. */
#ifndef ABAMD_GPU_HOST_H
#define ABAMD_GPU_HOST_H

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#define HIP_CHECK(x) do { hipError_t _e = (x); if (_e != hipSuccess) { \
    fprintf(stderr, "[abpoa_amd] HIP error %s at %s:%d: %s\n", hipGetErrorName(_e), __FILE__, __LINE__, hipGetErrorString(_e)); \
    exit(EXIT_FAILURE); } } while (0)

struct PinnedBuf {
    uint8_t *p = nullptr;
    size_t cap = 0;
    void ensure(size_t n) {
        if (n <= cap) return;
        size_t want = cap ? cap : 1 << 20;
        while (want < n) want <<= 1;
        if (p) HIP_CHECK(hipHostFree(p));
        HIP_CHECK(hipHostMalloc((void**)&p, want));
        cap = want;
    }
};

#endif
