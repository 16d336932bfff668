// Posterior-predictive moments fused into the branch x trunk contraction (vihmc_predict_moments).
//
// Replaces the post-processing that keeps every sample's prediction and reduces the list afterwards
// (Operator_network/VI_HMC/post_process_burgers.py:85-95 np.mean / np.std(pred_list, axis=0), :105-146 print_error,
// main_VI_HMC_burgers.py:183-241 predict_model's per-sample MSE): the [C, N, P] output of a batch of C samples is never
// written. A 256-thread workgroup owns one tile of 64 branch rows n x 128 trunk rows p (32 p per wave) of the [N][P]
// state and loops over the call's chains inside: for chain c it forms S_c = Z_b,c Z_t,c^T + b0_c for its tile on the
// fp32 MFMA with the operand roles and the k order of k_contract2's predict path (A = branch rows, B = trunk rows; full
// 16-wide blocks as k-permuted float4 reads, then the 4-wide tail steps), so every S is bit for bit the value
// vihmc_forward writes. The chain's 64 branch rows, which the four waves share, come through a double-buffered LDS
// image [64][W4] filled by LDS-DMA (no staging registers): chain c + 1's image is in flight under chain c's products.
// Each wave keeps its 32 trunk rows in registers for the chain. Every S is folded into per-lane fp64 accumulators
//     s1 += (double)S;  s2 += (double)S * (double)S        (the fp64 square of an fp32 value is exact)
// loaded from the state at tile start (accumulate != 0, else zero) and stored once at tile end. The additions run
// strictly in chain order into the running value, so a batch of 16 in one call and the same 16 in calls of 5 + 5 + 6
// leave identical bits; no floating-point atomics anywhere.
// The residual r = S - y (r = 0 where the plan's targets are masked and y is NaN, as on side A) gives, per (chain, n),
// the fp64 sum of r^2 over the tile's 128 p: DPP rotations round the 16-lane rows, then the 4 waves in order through LDS ->
// part[c][p tile][n]. k_moments_sse sums the p tiles in a fixed order into sse_rows[c][n] and each n tile's rows into
// a (sum r^2, 0) pair; k_contract_stats turns the chain's pairs into the likelihood.
// Every operand / target load is clamped to the last valid row, every state load and store is guarded by n < N, p < P.
#include "vihmc_bf16x6.h"
#include "vihmc_internal.h"

namespace vihmc {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma_m(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// The value as the compiler cannot trace it: index arithmetic derived from it is redone where it is used instead of
// living in registers across the chain loop (the loop-invariant target / state addresses of a lane's 32 elements
// would take ~130 VGPRs next to the 128 of the accumulators).
__device__ __forceinline__ int opaque(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

// v + (v of the lane N places round the 16-lane row): after N = 8, 4, 2, 1 every lane of a row holds the row's sum in
// one fixed order. Two 32-bit DPP moves and an add per step, no LDS round trip.
template <int N>
__device__ __forceinline__ double row_ror_add(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x120 + N, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x120 + N, 0xf, 0xf, false);
    return v + __hiloint2double(hi, lo);
}

// SNKB / SNTAIL as in k_contract2: >= 0 fixes the k-block structure at compile time (W = 100: 6 + 1), -1 reads it
// from W at run time. The run-time forms wider than 64 hold up to 8 + 3 owner registers per row more than fit beside
// the accumulators in 256 VGPRs: they run one workgroup per CU (512 VGPRs) instead of spilling.
template <int WMAX, int SNKB, int SNTAIL>
__global__ __launch_bounds__(256, (WMAX > 64 && SNKB < 0) ? 1 : 2) void k_predict_moments(MomentsProb P) {
    constexpr int NB = WMAX / 16;
    constexpr int QT = MOMENTS_TILE_N / 16;                 // 16-row branch sub-tiles per workgroup
    __shared__ double sh[2][4][MOMENTS_TILE_N];
    extern __shared__ float zbs[];                          // 2 x [MOMENTS_TILE_N][W4] branch rows of a chain
    const int W = P.W;
    const int W4 = (W + 3) & ~3;
    const int nkb = SNKB >= 0 ? SNKB : (W >> 4);
    const int ntail = SNTAIL >= 0 ? SNTAIL : ((W4 - (nkb << 4)) >> 2);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr0 = lane & 15, lg0 = lane >> 4;
    const int nt = blockIdx.x / P.p_tiles, pt = blockIdx.x - nt * P.p_tiles;
    const int n0 = nt * MOMENTS_TILE_N;
    const int o0 = pt * MOMENTS_TILE_P + wave * 32;
    // the branch-row image of one chain: W4 / 4 one-KB DMA pieces (64 lanes x 16 B), piece k = float4 64 k .. 64 k + 63
    // of the [64][W4 / 4] float4 image (rows past N: the last row again); wave w issues pieces w, w + 4, ...
    const int w4q = W4 >> 2;
    const int abuf = MOMENTS_TILE_N * W4;                   // floats per image
#define VIHMC_MOM_DMA(CH, BUF)                                                                               \
    for (int k = wave; k < w4q; k += 4) {                                                                    \
        const int e = 64 * k + lane, row = e / w4q, col = e - row * w4q;                                     \
        bf6::glds16_asm(P.Zb + (CH) * P.zb_cs + (int64_t)min(n0 + row, P.N - 1) * P.ldz + 4 * col,          \
                        zbs + (BUF) * abuf + 256 * k);                                                       \
    }

    // the state: zero, or (accumulate) loaded with the indices clamped to the last valid row / point (never stored there)
    double s1[QT][2][4], s2[QT][2][4];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        __builtin_amdgcn_sched_barrier(0);      // one sub-tile's 16 state accesses (and their addresses) at a time
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int r = 0; r < 4; ++r) s1[qt][s][r] = s2[qt][s][r] = 0.0;
        if (P.accumulate) {
            const int lr = opaque(lr0), lg = opaque(lg0);
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t i = (int64_t)min(n0 + 16 * qt + 4 * lg + r, P.N - 1) * P.P + min(o0 + 16 * s + lr, P.P - 1);
                    s1[qt][s][r] = P.sum1[i];
                    s2[qt][s][r] = P.sum2[i];
                }
        }
    }

    VIHMC_MOM_DMA(0, 0)
    // the targets of a sub-tile are loaded one sub-tile ahead (they do not depend on the chain: sub-tile 0's of the next
    // chain during sub-tile 3), so their latency hides under a sub-tile of MFMAs
    float yn[2][4];
#define VIHMC_MOM_YLOAD(QT)                                                                                   \
    {                                                                                                         \
        const int lr_ = opaque(lr0), lg_ = opaque(lg0);                                                       \
        _Pragma("unroll") for (int s = 0; s < 2; ++s)                                                         \
            _Pragma("unroll") for (int r = 0; r < 4; ++r)                                                     \
                yn[s][r] = P.Y[(int64_t)min(n0 + 16 * (QT) + 4 * lg_ + r, P.N - 1) * P.ldy +                  \
                               min(o0 + 16 * s + lr_, P.P - 1)];                                              \
    }
    VIHMC_MOM_YLOAD(0)
    bf6::wait_vmcnt0();
    __syncthreads();
    for (int c = 0; c < P.C; ++c) {
        // chain c + 1's image into the other buffer: its last readers (chain c - 1) are past the previous barrier
        if (c + 1 < P.C) {
            VIHMC_MOM_DMA(c + 1, (c + 1) & 1)
        }
        const float* Zt = P.Zt + c * P.zt_cs;
        const float* Zb = zbs + (c & 1) * abuf;
        const float b0 = P.b0[c * P.b0_cs];
        float4 ob[2][NB];
        float otl[2][3];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int lr = opaque(lr0), lg = opaque(lg0);
            const float* orow = Zt + (int64_t)min(o0 + 16 * s + lr, P.P - 1) * P.ldz;
#pragma unroll
            for (int bb = 0; bb < NB; ++bb)
                ob[s][bb] = (bb < nkb) ? *reinterpret_cast<const float4*>(orow + 16 * bb + 4 * lg)
                                       : float4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ts = 0; ts < 3; ++ts) otl[s][ts] = (ts < ntail) ? orow[16 * nkb + 4 * ts + lg] : 0.f;
        }
        double* shw = sh[c & 1][wave];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            const int lr = opaque(lr0), lg = opaque(lg0);
            const float* qrow = Zb + (16 * qt + lr) * W4;
            float yv[2][4];
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int r = 0; r < 4; ++r) yv[s][r] = yn[s][r];
            VIHMC_MOM_YLOAD((qt + 1) % QT)
            f32x4 sacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int bb = 0; bb < NB; ++bb) {
                if (bb < nkb) {
                    const float4 qa = *reinterpret_cast<const float4*>(qrow + 16 * bb + 4 * lg);
                    sacc[0] = mfma_m(qa.x, ob[0][bb].x, sacc[0]);
                    sacc[1] = mfma_m(qa.x, ob[1][bb].x, sacc[1]);
                    sacc[0] = mfma_m(qa.y, ob[0][bb].y, sacc[0]);
                    sacc[1] = mfma_m(qa.y, ob[1][bb].y, sacc[1]);
                    sacc[0] = mfma_m(qa.z, ob[0][bb].z, sacc[0]);
                    sacc[1] = mfma_m(qa.z, ob[1][bb].z, sacc[1]);
                    sacc[0] = mfma_m(qa.w, ob[0][bb].w, sacc[0]);
                    sacc[1] = mfma_m(qa.w, ob[1][bb].w, sacc[1]);
                }
            }
#pragma unroll
            for (int ts = 0; ts < 3; ++ts) {
                if (ts < ntail) {
                    const float qa = qrow[16 * nkb + 4 * ts + lg];
                    sacc[0] = mfma_m(qa, otl[0][ts], sacc[0]);
                    sacc[1] = mfma_m(qa, otl[1][ts], sacc[1]);
                }
            }
            double rr[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int nn = n0 + 16 * qt + 4 * lg + r, pp = o0 + 16 * s + lr;
                    const float sv = sacc[s][r] + b0;
                    const double d = (double)sv;
                    s1[qt][s][r] += d;
                    s2[qt][s][r] += d * d;
                    const float rv = sv - yv[s][r];
                    const bool okm = nn < P.N && pp < P.P && (!P.masked || yv[s][r] == yv[s][r]);   // NaN target: excluded
                    if (okm) rr[r] += (double)rv * (double)rv;
                }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                rr[r] = row_ror_add<1>(row_ror_add<2>(row_ror_add<4>(row_ror_add<8>(rr[r]))));
                if (lr == 0) shw[16 * qt + 4 * lg + r] = rr[r];
            }
        }
        // the barrier publishes chain c + 1's image (each wave has waited for its own pieces) and chain c's row sums;
        // the sums' buffer is rewritten by chain c + 2, after the barrier of chain c + 1 that its readers reach only
        // once they are done here
        bf6::wait_vmcnt0();
        __syncthreads();
        if (tid < MOMENTS_TILE_N && n0 + tid < P.N) {
            const double(*b)[MOMENTS_TILE_N] = sh[c & 1];
            P.part[((int64_t)c * P.p_tiles + pt) * P.N + n0 + tid] = ((b[0][tid] + b[1][tid]) + b[2][tid]) + b[3][tid];
        }
    }

#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        __builtin_amdgcn_sched_barrier(0);
        const int lr = opaque(lr0), lg = opaque(lg0);
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int nn = n0 + 16 * qt + 4 * lg + r, pp = o0 + 16 * s + lr;
                if (nn < P.N && pp < P.P) {
                    P.sum1[(int64_t)nn * P.P + pp] = s1[qt][s][r];
                    P.sum2[(int64_t)nn * P.P + pp] = s2[qt][s][r];
                }
            }
    }
}

// One workgroup per (n tile, chain): sse_rows[c][n] = sum over the p tiles of part[c][pt][n] -- four interleaved
// partial sums (p tiles q, q + 4, ... in order, q = 0..3), then the four in order -- and the tile's rows summed in
// order -> stats[c][n tile] = (sum r^2, 0), one "wave" of StatsJob's layout per n tile. Every order is fixed by the
// plan's shape alone.
__global__ __launch_bounds__(256) void k_moments_sse(MomentsProb P) {
    __shared__ double sh[4][MOMENTS_TILE_N];
    const int nt = blockIdx.x, c = blockIdx.y, tid = threadIdx.x, r = tid & (MOMENTS_TILE_N - 1), q = tid / MOMENTS_TILE_N;
    static_assert(MOMENTS_TILE_N == 64, "k_moments_sse: 4 x 64 threads");
    const int n = min(nt * MOMENTS_TILE_N + r, P.N - 1);
    const double* part = P.part + (int64_t)c * P.p_tiles * P.N + n;
    double t = 0.0;
    for (int pt = q; pt < P.p_tiles; pt += 4) t += part[(int64_t)pt * P.N];
    sh[q][r] = t;
    __syncthreads();
    if (q == 0) {
        t = ((sh[0][r] + sh[1][r]) + sh[2][r]) + sh[3][r];
        const bool ok = nt * MOMENTS_TILE_N + r < P.N;
        if (ok && P.sse_rows) P.sse_rows[(int64_t)c * P.N + n] = t;
        sh[0][r] = ok ? t : 0.0;
    }
    __syncthreads();
    if (tid == 0) {
        double tot = 0.0;
        for (int i = 0; i < MOMENTS_TILE_N; ++i) tot += sh[0][i];
        double* st = P.stats + c * P.stats_cs + 2 * nt;
        st[0] = tot;
        st[1] = 0.0;
    }
}

#undef VIHMC_MOM_DMA
#undef VIHMC_MOM_YLOAD

#define VIHMC_LAUNCH_M(kern)                                                          \
    do {                                                                              \
        hipLaunchKernelGGL(kern, dim3(p.n_tiles* p.p_tiles), dim3(256), shm, s, p);   \
        e = hipGetLastError();                                                        \
    } while (0)

hipError_t launch_predict_moments(const MomentsProb& p, hipStream_t s) {
    if (p.C < 1 || p.N < 1 || p.P < 1 || p.W < 1 || (int64_t)p.n_tiles * p.p_tiles > INT32_MAX) return hipErrorInvalidValue;
    hipError_t e = hipErrorInvalidValue;
    const int w = p.W;
    const size_t shm = sizeof(float) * 2 * MOMENTS_TILE_N * ((w + 3) & ~3);
    if (w == 100) VIHMC_LAUNCH_M((k_predict_moments<112, 6, 1>));
    else if (w <= 16) VIHMC_LAUNCH_M((k_predict_moments<16, -1, -1>));
    else if (w <= 32) VIHMC_LAUNCH_M((k_predict_moments<32, -1, -1>));
    else if (w <= 64) VIHMC_LAUNCH_M((k_predict_moments<64, -1, -1>));
    else if (w <= 112) VIHMC_LAUNCH_M((k_predict_moments<112, -1, -1>));
    else if (w <= 128) VIHMC_LAUNCH_M((k_predict_moments<128, -1, -1>));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_moments_sse, dim3(p.n_tiles, p.C), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace vihmc
