// Dropout of the train passes (include/fsmg.h "Dropout"): masks from a counter-based generator (Philox4x32-10), never
// stored -- forward and backward regenerate them.  Float4 grid-stride passes over the rows, wave64, one generator call per four
// elements, integer threshold compare, no LDS, no atomics.
#include <algorithm>
#include "fsmg_kernels.h"

namespace fsmg {
namespace {

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), the Random123 constants
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c;
}

// the four factors (scale or +0.0) of units 4 * j4 .. 4 * j4 + 3 of device row r
__device__ __forceinline__ float4 drop_factors(const DropArgs& a, uint32_t row, int j4) {
    const uint4 w = philox4x32_10(make_uint4((uint32_t)j4, row, a.site, a.pass), a.key0, a.key1);
    const int j = j4 << 2;
    float4 f;
    f.x = (j + 0 < a.W && (w.x >> 8) < a.thr) ? a.scale : 0.0f;
    f.y = (j + 1 < a.W && (w.y >> 8) < a.thr) ? a.scale : 0.0f;
    f.z = (j + 2 < a.W && (w.z >> 8) < a.thr) ? a.scale : 0.0f;
    f.w = (j + 3 < a.W && (w.w >> 8) < a.thr) ? a.scale : 0.0f;
    return f;
}

// a dropped element is +0.0 whatever it held (an infinity times zero would be a NaN)
__device__ __forceinline__ float4 apply_factors(float4 x, float4 f) {
#pragma clang fp contract(off)
    float4 y;
    y.x = f.x != 0.0f ? x.x * f.x : 0.0f; y.y = f.y != 0.0f ? x.y * f.y : 0.0f;
    y.z = f.z != 0.0f ? x.z * f.z : 0.0f; y.w = f.w != 0.0f ? x.w * f.w : 0.0f;
    return y;
}

// GATHER: row r of src is row ids[r] (the embedding rows of the pass's input ids); else row r.  dst may be src (backward, in place).
// Blocks of 64 x 4 threads: threadIdx.y picks the row (grid-stride over rows, four per block), the wave's 64 lanes walk the row's float4
// groups -- no division per element, one 32-bit remainder per row (variational), 1 KB contiguous per wave and step.  rows < 2^31.
__device__ __forceinline__ uint32_t counter_row(const DropArgs& a, uint32_t r) { return a.variational ? r % (uint32_t)a.B : r; }
template <bool GATHER>
__device__ __forceinline__ void dropout_body(const DropArgs& a, const float* src, const int* __restrict__ ids, float* dst) {
    const int ld4 = a.ld >> 2;
    const uint32_t rows = (uint32_t)a.rows;
    for (uint32_t r = blockIdx.x * 4u + threadIdx.y; r < rows; r += gridDim.x * 4u) {
        const uint32_t row = counter_row(a, r);
        const float4* s4 = reinterpret_cast<const float4*>(src + (GATHER ? (size_t)ids[r] : (size_t)r) * a.ld);
        float4* d4 = reinterpret_cast<float4*>(dst + (size_t)r * a.ld);
        for (int j4 = threadIdx.x; j4 < ld4; j4 += 64) d4[j4] = apply_factors(s4[j4], drop_factors(a, row, j4));
    }
}

__global__ __launch_bounds__(256) void k_dropout_fwd(const DropArgs a, const float* __restrict__ src, float* __restrict__ dst) {
    dropout_body<false>(a, src, nullptr, dst);
}
__global__ __launch_bounds__(256) void k_dropout_embed_fwd(const DropArgs a, const float* __restrict__ emb, const int* __restrict__ ids, float* __restrict__ dst) {
    dropout_body<true>(a, emb, ids, dst);
}
__global__ __launch_bounds__(256) void k_dropout_bwd(const DropArgs a, float* g) { dropout_body<false>(a, g, nullptr, g); }

// 0 / 1 bytes of a site, [rows][W] unpadded (tests)
__global__ __launch_bounds__(256) void k_dropout_mask(const DropArgs a, unsigned char* __restrict__ out) {
    const int w4 = (a.W + 3) >> 2;
    const uint32_t rows = (uint32_t)a.rows;
    for (uint32_t r = blockIdx.x * 4u + threadIdx.y; r < rows; r += gridDim.x * 4u) {
        const uint32_t row = counter_row(a, r);
        unsigned char* o = out + (size_t)r * a.W;
        for (int j4 = threadIdx.x; j4 < w4; j4 += 64) {
            const float4 f = drop_factors(a, row, j4);
            const float v[4] = {f.x, f.y, f.z, f.w};
            for (int q = 0; q < 4; ++q)
                if (4 * j4 + q < a.W) o[4 * j4 + q] = v[q] != 0.0f ? 1 : 0;
        }
    }
}

inline dim3 drop_block() { return dim3(64, 4, 1); }
inline int drop_grid(long long rows) { return (int)std::max<long long>(1, std::min<long long>((rows + 3) / 4, 256 * 8)); }
inline bool drop_ok(const DropArgs& a) { return a.rows >= 0 && a.rows < (1LL << 31) && a.W > 0 && a.ld >= a.W && (a.ld & 3) == 0 && a.B > 0; }

}  // namespace

hipError_t launch_dropout_fwd(hipStream_t s, const DropArgs& a, const float* src, float* dst) {
    if (!drop_ok(a) || !src || !dst) return hipErrorInvalidValue;
    if (a.rows == 0) return hipSuccess;
    k_dropout_fwd<<<drop_grid(a.rows), drop_block(), 0, s>>>(a, src, dst);
    return hipGetLastError();
}
hipError_t launch_dropout_embed_fwd(hipStream_t s, const DropArgs& a, const float* emb, const int* ids, float* dst) {
    if (!drop_ok(a) || !emb || !ids || !dst) return hipErrorInvalidValue;
    if (a.rows == 0) return hipSuccess;
    k_dropout_embed_fwd<<<drop_grid(a.rows), drop_block(), 0, s>>>(a, emb, ids, dst);
    return hipGetLastError();
}
hipError_t launch_dropout_bwd(hipStream_t s, const DropArgs& a, float* g) {
    if (!drop_ok(a) || !g) return hipErrorInvalidValue;
    if (a.rows == 0) return hipSuccess;
    k_dropout_bwd<<<drop_grid(a.rows), drop_block(), 0, s>>>(a, g);
    return hipGetLastError();
}
hipError_t launch_dropout_mask(hipStream_t s, const DropArgs& a, unsigned char* out) {
    if (!drop_ok(a) || !out) return hipErrorInvalidValue;
    if (a.rows == 0) return hipSuccess;
    k_dropout_mask<<<drop_grid(a.rows), drop_block(), 0, s>>>(a, out);
    return hipGetLastError();
}

}  // namespace fsmg
