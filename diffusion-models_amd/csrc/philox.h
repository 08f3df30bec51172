// Philox4x32-10 + Box-Muller: the library's N(0,1) stream (dm_randn).  Device code only; included by the translation
// units whose kernels draw noise in place (elementwise.hip, edm.hip), so that they all produce the same values.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dm {

__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
        uint32_t n1 = (uint32_t)p1;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        uint32_t n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}
__device__ __forceinline__ void philox_normal4(uint64_t seed, uint64_t draw, uint64_t idx4, float z[4]) {
    uint32_t c[4] = {(uint32_t)idx4, (uint32_t)(idx4 >> 32), (uint32_t)draw, (uint32_t)(draw >> 32)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float inv = 2.3283064365386963e-10f;  // 2^-32
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        float u1 = ((float)c[2 * h] + 1.0f) * inv;  // (0, 1]
        float u2 = (float)c[2 * h + 1] * inv;
        float rad = sqrtf(-2.0f * logf(fminf(u1, 1.0f)));
        float ang = 6.283185307179586f * u2;
        z[2 * h] = rad * cosf(ang);
        z[2 * h + 1] = rad * sinf(ang);
    }
}

}  // namespace dm
