// gm_eval.hip — per-step evaluation series (reference src/eval.py:245-486 create_routing_plots).
//
// One launch per evaluation step, one 256-thread block per env. The block reduces the env's two NetMon
// state tables [N][S] (the state the policy acted on at step t and at step t - 1) to the drift statistics
// of the reference (feature_diffs*: |cur - prev| in fp32, its mean over the nodes per state column, its
// mean and maximum over the table), and copies / reduces the step's per-env results (reward, info, the
// eval-only statistics, the per-packet detail of gm_step_detail) into row (e0 + env, t) of the caller's
// episode tables. Nothing is allocated; every table is written by exactly one block.
//
// Numerics: the difference and abs are fp32 (float32 numpy in the reference); every sum is fp64 in a fixed
// order: a thread adds its elements in node order, a wave combines its lanes with the xor butterfly, thread 0
// adds the waves in wave order; the column sums add their row groups in ascending order. No atomics: two
// runs on the same inputs write the same bits.
//
// State loads are 16-byte lanes: a row of S floats is S / 4 float4 chunks, lanes of a wave read consecutive
// chunks (64 lanes = 1 KB contiguous for S >= 256; whole rows back to back below that, the table being
// contiguous). S / 4 < 256: the block's 256 / (S / 4) row groups walk the nodes interleaved and their column
// partials meet in LDS; otherwise every thread owns whole columns.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/graph_marl_amd.h"

int gm_fail(int code, const std::string& msg);

namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int MAX_A = 64;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ float wave_max_f32(float v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ double wave_min_f64(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = fmin(v, __shfl_xor(v, m));
    return v;
}

struct Args {
    const float* cur;
    const float* prev;
    const float* reward;
    const uint8_t* done;
    const double* info;
    const double* eval;
    const int32_t* done_steps;
    const int32_t* done_opt;
    const uint8_t* success;
    double* series;
    double* fdiff;
    uint8_t* done_agents;
    double* dmap;
    long long e0;
    int N, S, A, t, T, D;
};

__global__ __launch_bounds__(TPB) void k_eval_series_step(Args a) {
    __shared__ double s_part[TPB * 4];  // column partials [row group][S] (S / 4 < 256: rg * S <= 1024)
    __shared__ double s_wsum[WAVES];
    __shared__ float s_wmax[WAVES];
    __shared__ double s_reward[MAX_A];
    __shared__ int s_key[MAX_A];  // distance-map key of a successful packet, -1 otherwise
    __shared__ int s_steps[MAX_A];
    __shared__ double s_spr_min;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const long long e = a.e0 + b;
    const int N = a.N, S = a.S, A = a.A;
    double* frow = a.fdiff + (e * a.T + a.t) * (long long)S;

    // ---- NetMon state drift ----
    double tsum = 0.0;
    float tmax = 0.0f;
    int RG = 1;
    if (a.cur) {
        const int CPR = S >> 2;                    // float4 chunks per row
        const int LPR = CPR < TPB ? CPR : TPB;     // threads across one row
        RG = TPB / LPR;                            // row groups (1 when a row needs the whole block)
        const int rg = tid / LPR, cl = tid - rg * LPR;
        const float4* cur = reinterpret_cast<const float4*>(a.cur + (long long)b * N * S);
        const float4* prev = a.prev ? reinterpret_cast<const float4*>(a.prev + (long long)b * N * S) : nullptr;
        if (rg < RG) {
            for (int c = cl; c < CPR; c += LPR) {
                double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll 4
                for (int n = rg; n < N; n += RG) {
                    const float4 x = cur[(long long)n * CPR + c];
                    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (prev) p = prev[(long long)n * CPR + c];
                    const float d0 = fabsf(x.x - p.x), d1 = fabsf(x.y - p.y), d2 = fabsf(x.z - p.z),
                                d3 = fabsf(x.w - p.w);
                    s0 += (double)d0;
                    s1 += (double)d1;
                    s2 += (double)d2;
                    s3 += (double)d3;
                    tmax = fmaxf(tmax, fmaxf(fmaxf(d0, d1), fmaxf(d2, d3)));
                }
                tsum += (s0 + s1) + (s2 + s3);
                if (RG == 1) {  // the thread owns these four columns
                    const double inv = 1.0 / (double)N;
                    double* o = frow + 4 * c;
                    o[0] = s0 * inv;
                    o[1] = s1 * inv;
                    o[2] = s2 * inv;
                    o[3] = s3 * inv;
                } else {
                    double* o = s_part + rg * S + 4 * c;
                    o[0] = s0;
                    o[1] = s1;
                    o[2] = s2;
                    o[3] = s3;
                }
            }
        }
    }
    tsum = wave_sum_f64(tsum);
    tmax = wave_max_f32(tmax);
    if (lane == 0) {
        s_wsum[wave] = tsum;
        s_wmax[wave] = tmax;
    }

    // ---- per-packet inputs (wave 0: lane = agent) ----
    if (wave == 0) {
        double spr = __longlong_as_double(0x7ff0000000000000LL);  // +inf
        if (lane < A) {
            const long long i = (long long)b * A + lane;
            s_reward[lane] = (double)a.reward[i];
            const int ok = a.success[i] != 0;
            const int steps = a.done_steps[i], opt = a.done_opt[i];
            s_steps[lane] = steps;
            s_key[lane] = ok ? (opt < 0 ? 0 : (opt < a.D - 1 ? opt : a.D - 1)) : -1;
            if (ok) spr = (double)steps / (double)opt;
            if (a.done[i]) a.done_agents[e * A + lane] = 1;
        }
        spr = wave_min_f64(spr);
        if (lane == 0) s_spr_min = spr;
    }
    __syncthreads();

    // ---- per-column means of the drift when row groups shared the columns ----
    if (a.cur) {
        if (RG > 1) {
            const double inv = 1.0 / (double)N;
            for (int j = tid; j < S; j += TPB) {
                double s = 0.0;
                for (int g = 0; g < RG; g++) s += s_part[g * S + j];
                frow[j] = s * inv;
            }
        }
    } else {
        for (int j = tid; j < S; j += TPB) frow[j] = 0.0;
    }

    // ---- distance map: thread d owns key d and adds its packets in agent order ----
    for (int d = tid; d < a.D; d += TPB) {
        double cnt = 0.0, sum = 0.0, sq = 0.0;
        for (int i = 0; i < A; i++) {
            if (s_key[i] == d) {
                const double v = (double)s_steps[i];
                cnt += 1.0;
                sum += v;
                sq += v * v;
            }
        }
        if (cnt > 0.0) {
            double* o = a.dmap + (e * a.D + d) * 3;
            o[0] += cnt;
            o[1] += sum;
            o[2] += sq;
        }
    }

    // ---- the series row ----
    if (tid < GM_SERIES_FIELDS) {
        double v;
        const double* info = a.info + (long long)b * GM_INFO_FIELDS;
        switch (tid) {
            case GM_SERIES_REWARD: {
                double s = 0.0;
                for (int i = 0; i < A; i++) s += s_reward[i];
                v = s / (double)A;
                break;
            }
            case GM_SERIES_THROUGHPUT: v = info[GM_INFO_THROUGHPUT]; break;
            case GM_SERIES_DROPPED: v = info[GM_INFO_DROPPED]; break;
            case GM_SERIES_BLOCKED: v = info[GM_INFO_BLOCKED]; break;
            case GM_SERIES_LOOPED: v = info[GM_INFO_LOOPED]; break;
            case GM_SERIES_N_ARRIVED: v = info[GM_INFO_N_ARRIVED]; break;
            case GM_SERIES_SUM_DELAYS_ARRIVED: v = info[GM_INFO_SUM_DELAYS_ARRIVED]; break;
            case GM_SERIES_SUM_SPR: v = info[GM_INFO_SUM_SPR]; break;
            case GM_SERIES_SPR_MIN: v = s_spr_min; break;
            case GM_SERIES_FEATURE_DIFFS_MEAN: {
                double s = 0.0;
                for (int w = 0; w < WAVES; w++) s += s_wsum[w];
                v = a.cur ? s / ((double)N * (double)S) : 0.0;
                break;
            }
            case GM_SERIES_FEATURE_DIFFS_MAX: {
                float m = 0.0f;
                for (int w = 0; w < WAVES; w++) m = fmaxf(m, s_wmax[w]);
                v = (double)m;
                break;
            }
            default:  // the five eval-only statistics, in GM_EVAL_* order
                v = a.eval ? a.eval[(long long)b * GM_EVAL_FIELDS + (tid - GM_SERIES_TOTAL_EDGE_LOAD)] : 0.0;
                break;
        }
        a.series[(e * a.T + a.t) * GM_SERIES_FIELDS + tid] = v;
    }
}

}  // namespace

extern "C" int gm_eval_series_step(const float* state_cur, const float* state_prev, int32_t n_env, int32_t n_nodes,
                                   int32_t state_size, const float* reward, const uint8_t* done, int32_t n_agents,
                                   const double* info, const double* eval, const int32_t* done_steps,
                                   const int32_t* done_opt, const uint8_t* success, int32_t t, int32_t n_steps,
                                   int64_t e0, int32_t n_active, int64_t n_episodes, double* series,
                                   double* feature_diffs, uint8_t* done_agents, double* distance_map,
                                   int32_t dist_bound, void* stream) {
    if (!reward || !done || !info || !done_steps || !done_opt || !success || !series || !feature_diffs ||
        !done_agents || !distance_map)
        return gm_fail(GM_ERR_INVALID_ARG, "gm_eval_series_step: null argument");
    if (n_env <= 0 || n_agents < 1 || n_agents > MAX_A || n_steps <= 0 || t < 0 || t >= n_steps || dist_bound < 2 ||
        n_active < 0 || n_active > n_env || e0 < 0 || e0 + n_active > n_episodes || state_size < 1)
        return gm_fail(GM_ERR_INVALID_ARG,
                       "gm_eval_series_step: bad sizes (1 <= n_agents <= 64, 0 <= t < n_steps, dist_bound >= 2, "
                       "n_active <= n_env, e0 + n_active <= n_episodes)");
    if (state_prev && !state_cur)
        return gm_fail(GM_ERR_INVALID_ARG, "gm_eval_series_step: state_prev without state_cur");
    if (state_cur) {
        if (n_nodes < 1 || n_nodes > 128 || state_size % 4 != 0 || state_size > 4096 ||
            (reinterpret_cast<uintptr_t>(state_cur) & 15) != 0 || (reinterpret_cast<uintptr_t>(state_prev) & 15) != 0)
            return gm_fail(GM_ERR_INVALID_ARG,
                           "gm_eval_series_step: state tables need 1 <= n_nodes <= 128, state_size % 4 == 0, "
                           "state_size <= 4096 and 16-byte aligned bases");
    }
    if (n_active == 0) return GM_OK;
    Args a;
    a.cur = state_cur;
    a.prev = state_prev;
    a.reward = reward;
    a.done = done;
    a.info = info;
    a.eval = eval;
    a.done_steps = done_steps;
    a.done_opt = done_opt;
    a.success = success;
    a.series = series;
    a.fdiff = feature_diffs;
    a.done_agents = done_agents;
    a.dmap = distance_map;
    a.e0 = e0;
    a.N = n_nodes;
    a.S = state_size;
    a.A = n_agents;
    a.t = t;
    a.T = n_steps;
    a.D = dist_bound;
    hipLaunchKernelGGL(k_eval_series_step, dim3(n_active), dim3(TPB), 0, (hipStream_t)stream, a);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess)
        return gm_fail(GM_ERR_HIP, std::string("gm_eval_series_step launch: ") + hipGetErrorString(err));
    return GM_OK;
}
