// gm_agents.hip — agent-communication ops of the DGN and CommNet agent models
// (reference src/model.py:45-117 AttModel, 747-794 CommNet) for the batched envs.
//
// Both are per-env A x A contractions with A <= 64 agents: far too small for MFMA tiles,
// so one workgroup per env stages the env's key/value (or hidden) rows in LDS and each
// thread owns (agent, head) or (agent, column) outputs. The projections around them
// (q/k/v, fc_out, LSTM) run on the GEMM kernels.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/graph_marl_amd.h"

int gm_fail(int code, const std::string& msg);

namespace {

constexpr int MAXA = 64;
constexpr int MAXD = 64;  // per-head key / value width

// AttModel core for one env per block: for agent i and head h,
//   w_ij = <q_i, k_j> / sqrt(dk)          (att_weights, returned before masking)
//   p_ij = softmax_j(adj_ij ? w_ij : -1e9)
//   out_i = sum_j p_ij v_j + v_i          (skip connection), heads concatenated
// q/k/v rows: [B*A][ld], head h at columns [h*d, (h+1)*d) of each.
// D > 0: dk == dv == D at compile time (the reference's 16: registers, unrolled);
// D == 0: runtime widths up to MAXD.
template <int D>
__global__ void k_agent_attention(const float* __restrict__ q, const float* __restrict__ k,
                                  const float* __restrict__ v, long long ld, const int8_t* __restrict__ adj, int A,
                                  int heads, int dk_, int dv_, float scale, float* __restrict__ out, long long ldo,
                                  float* __restrict__ wout) {
    constexpr int RD = D > 0 ? D : MAXD;
    const int dk = D > 0 ? D : dk_, dv = D > 0 ? D : dv_;
    extern __shared__ float sm[];
    const int b = blockIdx.x;
    float* ks = sm;                    // [A][heads*dk]
    float* vs = sm + A * heads * dk;   // [A][heads*dv]
    const int KD = heads * dk, VD = heads * dv;
    for (int idx = threadIdx.x; idx < A * KD; idx += blockDim.x) {
        const int j = idx / KD, c = idx - j * KD;
        ks[idx] = k[((long long)b * A + j) * ld + c];
    }
    for (int idx = threadIdx.x; idx < A * VD; idx += blockDim.x) {
        const int j = idx / VD, c = idx - j * VD;
        vs[idx] = v[((long long)b * A + j) * ld + c];
    }
    __syncthreads();
    const int8_t* ad = adj + (long long)b * A * A;
    for (int p = threadIdx.x; p < A * heads; p += blockDim.x) {
        const int i = p / heads, h = p - i * heads;
        float qi[RD];
        const float* qr = q + ((long long)b * A + i) * ld + h * dk;
#pragma unroll
        for (int d = 0; d < RD; d++)
            if (d < dk) qi[d] = qr[d];
        float mx = -INFINITY;
        for (int j = 0; j < A; j++) {
            const float* kj = ks + j * KD + h * dk;
            float s = 0.f;
#pragma unroll
            for (int d = 0; d < RD; d++)
                if (d < dk) s = fmaf(qi[d], kj[d], s);
            s *= scale;
            if (wout) wout[(((long long)b * heads + h) * A + i) * A + j] = s;
            mx = fmaxf(mx, ad[i * A + j] ? s : -1e9f);
        }
        float acc[RD];
#pragma unroll
        for (int d = 0; d < RD; d++) acc[d] = 0.f;
        float sum = 0.f;
        for (int j = 0; j < A; j++) {
            const float* kj = ks + j * KD + h * dk;
            float s = 0.f;
#pragma unroll
            for (int d = 0; d < RD; d++)
                if (d < dk) s = fmaf(qi[d], kj[d], s);
            s *= scale;
            const float e = expf((ad[i * A + j] ? s : -1e9f) - mx);
            sum += e;
            const float* vj = vs + j * VD + h * dv;
#pragma unroll
            for (int d = 0; d < RD; d++)
                if (d < dv) acc[d] = fmaf(e, vj[d], acc[d]);
        }
        const float inv = 1.0f / sum;
        const float* vi = vs + i * VD + h * dv;
        float* o = out + ((long long)b * A + i) * ldo + h * dv;
#pragma unroll
        for (int d = 0; d < RD; d++)
            if (d < dv) o[d] = acc[d] * inv + vi[d];
    }
}

// CommNet communication step for one env per block: out_i = h_i + mean_{j != i, adj_ij} h_j
// (count clamped to 1), src/model.py:780-787.
__global__ void k_agent_comm(const float* __restrict__ h, long long ldh, const int8_t* __restrict__ adj, int A, int H,
                             float* __restrict__ out, long long ldo) {
    __shared__ float inv[MAXA];
    const int b = blockIdx.x;
    const int8_t* ad = adj + (long long)b * A * A;
    for (int i = threadIdx.x; i < A; i += blockDim.x) {
        int cnt = 0;
        for (int j = 0; j < A; j++) cnt += (j != i && ad[i * A + j]) ? 1 : 0;
        inv[i] = 1.0f / (float)max(cnt, 1);
    }
    __syncthreads();
    const float* hb = h + (long long)b * A * ldh;
    for (int idx = threadIdx.x; idx < A * H; idx += blockDim.x) {
        const int i = idx / H, c = idx - i * H;
        float s = 0.f;
        for (int j = 0; j < A; j++)
            if (j != i && ad[i * A + j]) s += hb[(long long)j * ldh + c];
        out[((long long)b * A + i) * ldo + c] = hb[(long long)i * ldh + c] + s * inv[i];
    }
}

// Transpose of k_agent_comm (gm_agent_comm_bwd) for one env and one chunk of COMM_CH columns per block: with
// g = g0 + g1 (the x and h halves of a comm-round cell's input gradient),
//   dh_j = g_j + sum_{i != j, adj_ij} g_i / max(cnt_i, 1),  cnt_i = |{k != i : adj_ik}|,
// summed over i ascending in fp32. The block stages adj[b] in LDS, derives 1 / max(cnt_i, 1) per row and, per
// column j, the 64-bit set of the rows i that read j; every g row of the chunk is read from HBM once, summed into
// LDS, and each thread then owns V consecutive columns of an output row (V = 4: 16-byte lanes; V = 1: any base /
// stride). Plain vector stores only.
constexpr int COMM_CH = 128;

template <int V>
__global__ __launch_bounds__(256) void k_agent_comm_bwd(const float* __restrict__ g0, long long ld0,
                                                        const float* __restrict__ g1, long long ld1,
                                                        const int8_t* __restrict__ adj, int A, int H,
                                                        float* __restrict__ dh, long long ldd) {
    __shared__ __attribute__((aligned(16))) float gs[MAXA * COMM_CH];
    __shared__ int8_t sadj[MAXA * MAXA];
    __shared__ float inv[MAXA];
    __shared__ unsigned long long readers[MAXA];
    const int b = blockIdx.x;
    const int c0 = blockIdx.y * COMM_CH;
    const int cw = min(COMM_CH, H - c0);  // columns of this chunk (V = 4: H % 4 == 0, so cw % 4 == 0)
    const int nv = cw / V;
    const int8_t* ad = adj + (long long)b * A * A;
    for (int idx = threadIdx.x; idx < A * A; idx += blockDim.x) sadj[idx] = ad[idx];
    const long long row0 = (long long)b * A;
    for (int idx = threadIdx.x; idx < A * nv; idx += blockDim.x) {
        const int i = idx / nv, c = (idx - i * nv) * V;
        const float* p0 = g0 + (row0 + i) * ld0 + c0 + c;
        if constexpr (V == 4) {
            float4 v = *reinterpret_cast<const float4*>(p0);
            if (g1) {
                const float4 w = *reinterpret_cast<const float4*>(g1 + (row0 + i) * ld1 + c0 + c);
                v.x += w.x;
                v.y += w.y;
                v.z += w.z;
                v.w += w.w;
            }
            *reinterpret_cast<float4*>(gs + i * COMM_CH + c) = v;
        } else {
            float v = p0[0];
            if (g1) v += g1[(row0 + i) * ld1 + c0 + c];
            gs[i * COMM_CH + c] = v;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < A; i += blockDim.x) {
        int cnt = 0;
        unsigned long long rd = 0ull;
        for (int k = 0; k < A; k++) {
            cnt += (k != i && sadj[i * A + k]) ? 1 : 0;
            if (k != i && sadj[k * A + i]) rd |= 1ull << k;  // row k reads column i
        }
        inv[i] = 1.0f / (float)max(cnt, 1);
        readers[i] = rd;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < A * nv; idx += blockDim.x) {
        const int j = idx / nv, c = (idx - j * nv) * V;
        unsigned long long rd = readers[j];
        float* o = dh + (row0 + j) * ldd + c0 + c;
        if constexpr (V == 4) {
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
            while (rd) {  // ascending i
                const int i = __ffsll(rd) - 1;
                rd &= rd - 1;
                const float f = inv[i];
                const float4 v = *reinterpret_cast<const float4*>(gs + i * COMM_CH + c);
                s.x = fmaf(v.x, f, s.x);
                s.y = fmaf(v.y, f, s.y);
                s.z = fmaf(v.z, f, s.z);
                s.w = fmaf(v.w, f, s.w);
            }
            const float4 own = *reinterpret_cast<const float4*>(gs + j * COMM_CH + c);
            *reinterpret_cast<float4*>(o) = make_float4(own.x + s.x, own.y + s.y, own.z + s.z, own.w + s.w);
        } else {
            float s = 0.f;
            while (rd) {
                const int i = __ffsll(rd) - 1;
                rd &= rd - 1;
                s = fmaf(gs[i * COMM_CH + c], inv[i], s);
            }
            o[0] = gs[j * COMM_CH + c] + s;
        }
    }
}

int launched(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return gm_fail(GM_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return GM_OK;
}

}  // namespace

extern "C" int gm_agent_attention(const float* q, const float* k, const float* v, int64_t ld, const int8_t* adj,
                                  int32_t B, int32_t A, int32_t heads, int32_t dk, int32_t dv, float* out,
                                  int64_t ldo, float* att_weights, void* stream) {
    if (!q || !k || !v || !adj || !out || B <= 0 || A <= 0 || A > MAXA || heads <= 0 || dk <= 0 || dk > MAXD ||
        dv <= 0 || dv > MAXD || ld < (int64_t)heads * (dk > dv ? dk : dv) || ldo < (int64_t)heads * dv)
        return gm_fail(GM_ERR_INVALID_ARG, "gm_agent_attention: bad arguments (A <= 64, dk, dv <= 64)");
    const size_t lds = (size_t)A * heads * (dk + dv) * sizeof(float);
    if (lds > 160 * 1024) return gm_fail(GM_ERR_UNSUPPORTED, "gm_agent_attention: A * heads * (dk + dv) too large");
    const float scale = 1.0f / sqrtf((float)dk);
    if (dk == 16 && dv == 16)
        hipLaunchKernelGGL(k_agent_attention<16>, dim3(B), dim3(256), lds, (hipStream_t)stream, q, k, v,
                           (long long)ld, adj, A, heads, dk, dv, scale, out, (long long)ldo, att_weights);
    else
        hipLaunchKernelGGL(k_agent_attention<0>, dim3(B), dim3(256), lds, (hipStream_t)stream, q, k, v,
                           (long long)ld, adj, A, heads, dk, dv, scale, out, (long long)ldo, att_weights);
    return launched("gm_agent_attention");
}

extern "C" int gm_agent_comm(const float* h, int64_t ldh, const int8_t* adj, int32_t B, int32_t A, int32_t H,
                             float* out, int64_t ldo, void* stream) {
    if (!h || !adj || !out || B <= 0 || A <= 0 || A > MAXA || H <= 0 || ldh < H || ldo < H || h == out)
        return gm_fail(GM_ERR_INVALID_ARG, "gm_agent_comm: bad arguments (A <= 64, out must not alias h)");
    hipLaunchKernelGGL(k_agent_comm, dim3(B), dim3(256), 0, (hipStream_t)stream, h, (long long)ldh, adj, A, H, out,
                       (long long)ldo);
    return launched("gm_agent_comm");
}

extern "C" int gm_agent_comm_bwd(const float* g0, int64_t ld0, const float* g1, int64_t ld1, const int8_t* adj,
                                 int32_t B, int32_t A, int32_t H, float* dh, int64_t ldd, void* stream) {
    if (!g0 || !adj || !dh || B <= 0 || A <= 0 || H <= 0 || ld0 < H || (g1 && ld1 < H) || ldd < H || dh == g0 ||
        dh == g1)
        return gm_fail(GM_ERR_INVALID_ARG, "gm_agent_comm_bwd: bad arguments (dh must not alias g0 or g1)");
    if (A > MAXA || H > 1024)
        return gm_fail(GM_ERR_UNSUPPORTED, "gm_agent_comm_bwd: A <= 64 and H <= 1024 only");
    auto a16 = [](const void* p, int64_t ld) { return !p || ((reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0); };
    const dim3 grid((unsigned)B, (unsigned)((H + COMM_CH - 1) / COMM_CH));
    if (H % 4 == 0 && a16(g0, ld0) && a16(g1, ld1) && a16(dh, ldd))
        hipLaunchKernelGGL(k_agent_comm_bwd<4>, grid, dim3(256), 0, (hipStream_t)stream, g0, (long long)ld0, g1,
                           (long long)ld1, adj, A, H, dh, (long long)ldd);
    else
        hipLaunchKernelGGL(k_agent_comm_bwd<1>, grid, dim3(256), 0, (hipStream_t)stream, g0, (long long)ld0, g1,
                           (long long)ld1, adj, A, H, dh, (long long)ldd);
    return launched("gm_agent_comm_bwd");
}
