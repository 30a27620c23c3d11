// fc_bwd.hip -- the elementwise part of a fully-connected layer's backward, in ONE pass over the rows (the released VGGish
// embedding layers, audio_backbone._ReleasedEmbeddings):
//
//     dz = a <= 0 ? 0 : da       (torch's ReLU backward on the SAVED post-ReLU output a: a zero activation stops any gradient,
//                                 a NaN activation lets it through; no mask when a is absent: the output layer)
//     dz -> split bf16 planes hi / lo (the operand of the bf16x3 weight / data gradient) and / or fp32 (the fp32 mode)
//     db = column sums of dz     (per-slab partials here, folded by a second small launch in slab order)
//
// Separately these are three launches and three HBM round trips (act_mask_bwd, col_sum, split_bf16).  Blocks are
// 32 column lanes x 8 row lanes over a slab of rows; each lane owns CPT consecutive columns (8: one 16-byte load / store
// per 16-bit plane, two per fp32 tensor; 4 when C % 8 != 0).  Every sum runs in a fixed order (rows of a lane in increasing
// order, the 8 row lanes in order, the slabs in order): no atomics, bit-identical from run to run.
#include <stdint.h>

#include "conv_common.h"

namespace cer {

constexpr int FC_TX = 32, FC_TY = 8, FC_UNROLL = 4;

template <int CPT> __device__ __forceinline__ void load_u16(const uint16_t *p, uint16_t v[CPT]) {
    if constexpr (CPT == 8) {
        const uint4 q = *reinterpret_cast<const uint4 *>(p);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[2 * i] = (uint16_t)(w[i] & 0xffffu); v[2 * i + 1] = (uint16_t)(w[i] >> 16); }
    } else {
        const ushort4 q = *reinterpret_cast<const ushort4 *>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
}

template <int CPT> __device__ __forceinline__ void store_u16(uint16_t *p, const uint16_t v[CPT]) {
    if constexpr (CPT == 8) {
        uint4 q;
        q.x = v[0] | ((uint32_t)v[1] << 16); q.y = v[2] | ((uint32_t)v[3] << 16);
        q.z = v[4] | ((uint32_t)v[5] << 16); q.w = v[6] | ((uint32_t)v[7] << 16);
        *reinterpret_cast<uint4 *>(p) = q;
    } else {
        ushort4 q;
        q.x = v[0]; q.y = v[1]; q.z = v[2]; q.w = v[3];
        *reinterpret_cast<ushort4 *>(p) = q;
    }
}

// the saved activation of row r, columns c0 .. c0 + CPT - 1, as fp32 values (only a <= 0 is tested: NaN is not)
template <int CPT, int KIND>
__device__ __forceinline__ void load_act(const void *a, const uint16_t *alo, size_t off, float v[CPT]) {
    if constexpr (KIND == CER_FC_ACT_F32) {
#pragma unroll
        for (int i = 0; i < CPT; i += 4) {
            const float4 q = *reinterpret_cast<const float4 *>((const float *)a + off + i);
            v[i] = q.x; v[i + 1] = q.y; v[i + 2] = q.z; v[i + 3] = q.w;
        }
    } else if constexpr (KIND == CER_FC_ACT_SPLIT) {
        uint16_t h[CPT], l[CPT];
        load_u16<CPT>((const uint16_t *)a + off, h);
        load_u16<CPT>(alo + off, l);
#pragma unroll
        for (int i = 0; i < CPT; ++i) v[i] = bf16_to_f32(h[i]) + bf16_to_f32(l[i]);
    } else if constexpr (KIND == CER_FC_ACT_BF16 || KIND == CER_FC_ACT_F16) {
        uint16_t h[CPT];
        load_u16<CPT>((const uint16_t *)a + off, h);
#pragma unroll
        for (int i = 0; i < CPT; ++i) v[i] = KIND == CER_FC_ACT_F16 ? f16_to_f32(h[i]) : bf16_to_f32(h[i]);
    } else {
#pragma unroll
        for (int i = 0; i < CPT; ++i) v[i] = 1.f;
    }
}

template <int CPT, bool VEC, int KIND>
__global__ __launch_bounds__(256) void fc_bwd_elem_kernel(const float *__restrict__ da, int ld, const void *__restrict__ a,
                                                          const uint16_t *__restrict__ alo, uint16_t *__restrict__ zhi,
                                                          uint16_t *__restrict__ zlo, float *__restrict__ z32,
                                                          float *__restrict__ part, int R, int C, int rows_per_slab) {
    constexpr int BC = FC_TX * CPT;
    __shared__ float red[FC_TY][BC];
    const int tx = threadIdx.x % FC_TX, ty = threadIdx.x / FC_TX;
    const int c0 = blockIdx.x * BC + tx * CPT;
    const int r_begin = blockIdx.y * rows_per_slab, r_end = min(R, r_begin + rows_per_slab);
    float acc[CPT];
#pragma unroll
    for (int i = 0; i < CPT; ++i) acc[i] = 0.f;
    if (c0 < C) {   // C % CPT == 0: a lane's columns are all in range or all out
        for (int r0 = r_begin + ty; r0 < r_end; r0 += FC_TY * FC_UNROLL) {
            float d[FC_UNROLL][CPT], m[FC_UNROLL][CPT];
#pragma unroll
            for (int u = 0; u < FC_UNROLL; ++u) {   // all loads of the batch first: FC_UNROLL rows in flight per lane
                const int r = r0 + u * FC_TY;
                if (r < r_end) {
                    const float *src = da + (size_t)r * ld + c0;
                    if constexpr (VEC) {
#pragma unroll
                        for (int i = 0; i < CPT; i += 4) {
                            const float4 q = *reinterpret_cast<const float4 *>(src + i);
                            d[u][i] = q.x; d[u][i + 1] = q.y; d[u][i + 2] = q.z; d[u][i + 3] = q.w;
                        }
                    } else {
#pragma unroll
                        for (int i = 0; i < CPT; ++i) d[u][i] = src[i];
                    }
                    load_act<CPT, KIND>(a, alo, (size_t)r * C + c0, m[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < FC_UNROLL; ++u) {
                const int r = r0 + u * FC_TY;
                if (r < r_end) {
                    float z[CPT];
#pragma unroll
                    for (int i = 0; i < CPT; ++i) {
                        // a select, not a product: a zero activation stops a non-finite incoming gradient like ReLU's backward,
                        // and a NaN activation lets the gradient through (torch's threshold_backward: a <= 0 ? 0 : g)
                        z[i] = m[u][i] <= 0.f ? 0.f : d[u][i];
                        acc[i] += z[i];
                    }
                    const size_t off = (size_t)r * C + c0;
                    if (zhi) {
                        uint16_t h[CPT], l[CPT];
#pragma unroll
                        for (int i = 0; i < CPT; ++i) split_bf16(z[i], h[i], l[i]);
                        store_u16<CPT>(zhi + off, h);
                        store_u16<CPT>(zlo + off, l);
                    }
                    if (z32) {
#pragma unroll
                        for (int i = 0; i < CPT; i += 4)
                            *reinterpret_cast<float4 *>(z32 + off + i) = make_float4(z[i], z[i + 1], z[i + 2], z[i + 3]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < CPT; ++i) red[ty][tx * CPT + i] = acc[i];
    __syncthreads();
    for (int j = threadIdx.x; j < BC; j += blockDim.x) {
        const int c = blockIdx.x * BC + j;
        if (c < C) {
            float s = red[0][j];
#pragma unroll
            for (int t = 1; t < FC_TY; ++t) s += red[t][j];
            part[(size_t)blockIdx.y * C + c] = s;
        }
    }
}

// db[c] = sum over the slabs, in slab order
__global__ __launch_bounds__(256) void fc_bwd_db_kernel(const float *__restrict__ part, float *__restrict__ db, int slabs, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float s = 0.f;
#pragma unroll 8
    for (int k = 0; k < slabs; ++k) s += part[(size_t)k * C + c];
    db[c] = s;
}

// rows per slab: 32 (four rows per row lane, enough blocks to fill the chip at R = 1024), doubled until at most 256 slabs
static int fc_rows_per_slab(int R) {
    int rps = 32;
    while ((R + rps - 1) / rps > 256) rps *= 2;
    return rps;
}

template <int CPT, bool VEC>
static void fc_launch_kind(int kind, dim3 grid, hipStream_t st, const float *da, int ld, const void *a, const uint16_t *alo,
                           uint16_t *zhi, uint16_t *zlo, float *z32, float *part, int R, int C, int rps) {
#define FC_CASE(K)                                                                                                        \
    case K:                                                                                                               \
        CER_LAUNCH((fc_bwd_elem_kernel<CPT, VEC, K>), grid, dim3(256), 0, st, da, ld, a, alo, zhi, zlo, z32, part, R, C, \
                   rps);                                                                                                  \
        break;
    switch (kind) {
        FC_CASE(CER_FC_ACT_NONE)
        FC_CASE(CER_FC_ACT_F32)
        FC_CASE(CER_FC_ACT_SPLIT)
        FC_CASE(CER_FC_ACT_BF16)
        FC_CASE(CER_FC_ACT_F16)
    }
#undef FC_CASE
}

static inline bool fc_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace cer

using namespace cer;

extern "C" size_t cer_fc_bwd_workspace_bytes(int R, int C) {
    if (R <= 0 || C <= 0) return 0;
    const int slabs = (R + fc_rows_per_slab(R) - 1) / fc_rows_per_slab(R);
    return slabs > 1 ? (size_t)slabs * C * sizeof(float) : 0;
}

extern "C" int cer_fc_bwd_elem(const float *da, int da_ld, const void *a, const uint16_t *a_lo, int a_kind, uint16_t *dz_hi,
                               uint16_t *dz_lo, float *dz, float *db, int R, int C, void *workspace, size_t workspace_bytes,
                               void *stream) {
    if (!da || !db || R <= 0 || C <= 0 || (C & 3) || da_ld < C)
        return cer_set_error(CER_ERR_INVALID_ARG, "fc_bwd_elem: needs da, db, R >= 1, C %% 4 == 0 and da_ld >= C");
    if (a_kind < CER_FC_ACT_NONE || a_kind > CER_FC_ACT_F16 || (a_kind != CER_FC_ACT_NONE) != (a != nullptr) ||
        (a_kind == CER_FC_ACT_SPLIT) != (a_lo != nullptr))
        return cer_set_error(CER_ERR_INVALID_ARG, "fc_bwd_elem: the activation pointers do not match a_kind");
    if ((dz_hi == nullptr) != (dz_lo == nullptr) || (!dz_hi && !dz))
        return cer_set_error(CER_ERR_INVALID_ARG, "fc_bwd_elem: give the split planes (hi and lo), the fp32 dz, or both");
    if (!fc_aligned16(a) || !fc_aligned16(a_lo) || !fc_aligned16(dz_hi) || !fc_aligned16(dz_lo) || !fc_aligned16(dz))
        return cer_set_error(CER_ERR_INVALID_ARG, "fc_bwd_elem: the activation and output tensors must be 16-byte aligned");
    const int rps = fc_rows_per_slab(R);
    const int slabs = (R + rps - 1) / rps;
    float *part = db;
    if (slabs > 1) {
        if (!workspace || workspace_bytes < (size_t)slabs * C * sizeof(float) || !fc_aligned16(workspace))
            return cer_set_error(CER_ERR_WORKSPACE, "fc_bwd_elem: workspace too small (cer_fc_bwd_workspace_bytes)");
        part = (float *)workspace;
    }
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (da_ld & 3) == 0 && fc_aligned16(da);   // otherwise dA is read element by element (any ld >= C)
    if ((C & 7) == 0) {
        const dim3 grid((C + FC_TX * 8 - 1) / (FC_TX * 8), slabs);
        if (vec) fc_launch_kind<8, true>(a_kind, grid, st, da, da_ld, a, a_lo, dz_hi, dz_lo, dz, part, R, C, rps);
        else fc_launch_kind<8, false>(a_kind, grid, st, da, da_ld, a, a_lo, dz_hi, dz_lo, dz, part, R, C, rps);
    } else {
        const dim3 grid((C + FC_TX * 4 - 1) / (FC_TX * 4), slabs);
        if (vec) fc_launch_kind<4, true>(a_kind, grid, st, da, da_ld, a, a_lo, dz_hi, dz_lo, dz, part, R, C, rps);
        else fc_launch_kind<4, false>(a_kind, grid, st, da, da_ld, a, a_lo, dz_hi, dz_lo, dz, part, R, C, rps);
    }
    CER_HIP_CHECK(hipGetLastError());
    if (slabs > 1) {
        CER_LAUNCH(fc_bwd_db_kernel, dim3((C + 255) / 256), dim3(256), 0, st, (const float *)part, db, slabs, C);
        CER_HIP_CHECK(hipGetLastError());
    }
    return CER_OK;
}
