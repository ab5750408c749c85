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
#include "gm_device.hpp"

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

// Transpose of the k_agent_attention core (gm_agent_attention_bwd) for one env per block. With, per (agent i, head),
//   w_ij = <q_i, k_j> / sqrt(dk),  p_i. = softmax_j(adj_ij ? w_ij : -1e9),  dP_ij = <dout_i, v_j>,
//   Ds_i = sum_j p_ij dP_ij,       dw_ij = adj_ij ? p_ij (dP_ij - Ds_i) : 0    (masked_fill passes no gradient),
// and, with the regulariser (REG: the target model's q_tar / k_tar rows, row scale r, 1 when null),
//   dw_ij += r_i (softmax_j(w_i.) - softmax_j(w_tar,i.))_j                     over ALL j (unmasked softmaxes),
// the outputs are dq_i = sum_j dw_ij k_j / sqrt(dk), dk_j = sum_i dw_ij q_i / sqrt(dk), dv_j = sum_i p_ij dout_i +
// dout_j (skip connection). Phase 1 stages the env's k, v (and k_tar) rows and adj in LDS: a thread owns (i, head),
// reads its own q_i, dout_i (q_tar,i) rows from HBM, keeps the row statistics (max, 1 / sum, Ds; REG: the two
// unmasked softmaxes' max and 1 / sum, r_i) in LDS and writes dq_i. Phase 2 stages q, dout (and q_tar) over the same
// LDS: a thread owns (j, head), reads its own k_j, v_j (k_tar,j) rows, recomputes p_ij and dw_ij from the statistics
// for i ascending and sums dk_j, dv_j in fp32 registers: no A x A array anywhere, no atomics, the same bits on every
// run. LDS per env: A heads ((REG ? 2 : 1) dk + dv + (REG ? 8 : 3)) floats + A^2 bytes (37 KB at A = 20, 8 heads,
// d = 16 with the regulariser: 4 envs per CU). Plain vector stores.
template <int D, bool REG>
__global__ __launch_bounds__(256) void k_agent_attention_bwd(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, long long ld,
    const int8_t* __restrict__ adj, int A, int heads, int dk_, int dv_, float scale, const float* __restrict__ dout,
    long long ldo, const float* __restrict__ qt, const float* __restrict__ kt, long long ldt,
    const float* __restrict__ r, float* __restrict__ dq, float* __restrict__ dkk, float* __restrict__ dvv,
    long long ldd) {
    constexpr int RD = D > 0 ? D : MAXD;
    constexpr int NS = REG ? 8 : 3;
    const int dk = D > 0 ? D : dk_, dv = D > 0 ? D : dv_;
    extern __shared__ float sm[];
    const int b = blockIdx.x;
    const int KD = heads * dk, VD = heads * dv;
    float* ks = sm;               // [A][KD]  phase 1: k,     phase 2: q
    float* vs = ks + A * KD;      // [A][VD]  phase 1: v,     phase 2: dout
    float* kts = vs + A * VD;     // [A][KD]  phase 1: k_tar, phase 2: q_tar (REG)
    float* st = kts + (REG ? A * KD : 0);  // [A * heads][NS]
    int8_t* sadj = reinterpret_cast<int8_t*>(st + A * heads * NS);
    float *qs = ks, *ds = vs, *qts = kts;
    const long long row0 = (long long)b * A;
    for (int idx = threadIdx.x; idx < A * KD; idx += blockDim.x) {
        const int j = idx / KD, c = idx - j * KD;
        ks[idx] = k[(row0 + j) * ld + c];
        if (REG) kts[idx] = kt[(row0 + j) * ldt + c];
    }
    for (int idx = threadIdx.x; idx < A * VD; idx += blockDim.x) {
        const int j = idx / VD, c = idx - j * VD;
        vs[idx] = v[(row0 + j) * ld + c];
    }
    for (int idx = threadIdx.x; idx < A * A; idx += blockDim.x) sadj[idx] = adj[row0 * A + idx];
    __syncthreads();

    // ---- phase 1: (i, head) rows: statistics and dq_i ----
    for (int p = threadIdx.x; p < A * heads; p += blockDim.x) {
        const int i = p / heads, h = p - i * heads;
        float qi[RD], di[RD];
#pragma unroll
        for (int d = 0; d < RD; d++) {
            if (d < dk) qi[d] = q[(row0 + i) * ld + h * dk + d];
            if (d < dv) di[d] = dout[(row0 + i) * ldo + h * dv + d];
        }
        // (REG) the thread's own q_tar row: registers at the compile-time width, read in place otherwise
        float qtr[D > 0 ? D : 1];
        const float* qti = REG ? qt + (row0 + i) * ldt + h * dk : nullptr;
        if constexpr (D > 0 && REG) {
#pragma unroll
            for (int d = 0; d < D; d++) qtr[d] = qti[d];
            qti = qtr;
        }
        const int8_t* ai = sadj + i * A;
        float mx = -INFINITY, mxu = -INFINITY, mxt = -INFINITY;
        for (int j = 0; j < A; j++) {
            const float* kj = ks + j * KD + h * dk;
            float s = 0.f;
#pragma unroll
            for (int d = 0; d < RD; d++)
                if (d < dk) s = fmaf(qi[d], kj[d], s);
            s *= scale;
            mx = fmaxf(mx, ai[j] ? s : -1e9f);
            if (REG) {
                const float* ktj = kts + j * KD + h * dk;
                float t = 0.f;
#pragma unroll
                for (int d = 0; d < RD; d++)
                    if (d < dk) t = fmaf(qti[d], ktj[d], t);
                mxu = fmaxf(mxu, s);
                mxt = fmaxf(mxt, t * scale);
            }
        }
        float sum = 0.f, num = 0.f, sumu = 0.f, sumt = 0.f;
        for (int j = 0; j < A; j++) {
            const float* kj = ks + j * KD + h * dk;
            const float* vj = vs + j * VD + h * dv;
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < RD; d++)
                if (d < dk) s = fmaf(qi[d], kj[d], s);
#pragma unroll
            for (int d = 0; d < RD; d++)
                if (d < dv) dp = fmaf(di[d], vj[d], dp);
            s *= scale;
            const float e = expf((ai[j] ? s : -1e9f) - mx);
            sum += e;
            num = fmaf(e, dp, num);
            if (REG) {
                const float* ktj = kts + j * KD + h * dk;
                float t = 0.f;
#pragma unroll
                for (int d = 0; d < RD; d++)
                    if (d < dk) t = fmaf(qti[d], ktj[d], t);
                sumu += expf(s - mxu);
                sumt += expf(t * scale - mxt);
            }
        }
        const float inv = 1.0f / sum, Ds = num * inv;
        const float invu = REG ? 1.0f / sumu : 0.f, invt = REG ? 1.0f / sumt : 0.f;
        const float ri = REG ? (r ? r[row0 + i] : 1.0f) : 0.f;
        float* sp = st + p * NS;
        sp[0] = mx;
        sp[1] = inv;
        sp[2] = Ds;
        if (REG) {
            sp[3] = mxu;
            sp[4] = invu;
            sp[5] = mxt;
            sp[6] = invt;
            sp[7] = ri;
        }
        float acc[RD];
#pragma unroll
        for (int d = 0; d < RD; d++) acc[d] = 0.f;
        for (int j = 0; j < A; j++) {
            const float* kj = ks + j * KD + h * dk;
            const float* vj = vs + j * VD + h * dv;
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < RD; d++)
                if (d < dk) s = fmaf(qi[d], kj[d], s);
#pragma unroll
            for (int d = 0; d < RD; d++)
                if (d < dv) dp = fmaf(di[d], vj[d], dp);
            s *= scale;
            float dw = 0.f;
            if (ai[j]) dw = expf(s - mx) * inv * (dp - Ds);
            if (REG) {
                const float* ktj = kts + j * KD + h * dk;
                float t = 0.f;
#pragma unroll
                for (int d = 0; d < RD; d++)
                    if (d < dk) t = fmaf(qti[d], ktj[d], t);
                dw += ri * (expf(s - mxu) * invu - expf(t * scale - mxt) * invt);
            }
#pragma unroll
            for (int d = 0; d < RD; d++)
                if (d < dk) acc[d] = fmaf(dw, kj[d], acc[d]);
        }
        float* o = dq + (row0 + i) * ldd + h * dk;
#pragma unroll
        for (int d = 0; d < RD; d++)
            if (d < dk) o[d] = acc[d] * scale;
    }
    __syncthreads();

    // ---- phase 2: q, dout (q_tar) over the rows phase 1 read; (j, head) columns: dk_j, dv_j over i ascending ----
    for (int idx = threadIdx.x; idx < A * KD; idx += blockDim.x) {
        const int j = idx / KD, c = idx - j * KD;
        qs[idx] = q[(row0 + j) * ld + c];
        if (REG) qts[idx] = qt[(row0 + j) * ldt + c];
    }
    for (int idx = threadIdx.x; idx < A * VD; idx += blockDim.x) {
        const int j = idx / VD, c = idx - j * VD;
        ds[idx] = dout[(row0 + j) * ldo + c];
    }
    __syncthreads();
    for (int p = threadIdx.x; p < A * heads; p += blockDim.x) {
        const int j = p / heads, h = p - j * heads;
        float kj[RD], vj[RD], ak[RD], av[RD];
#pragma unroll
        for (int d = 0; d < RD; d++) {
            if (d < dk) kj[d] = k[(row0 + j) * ld + h * dk + d];
            if (d < dv) vj[d] = v[(row0 + j) * ld + h * dv + d];
            ak[d] = 0.f;
            av[d] = 0.f;
        }
        float ktr[D > 0 ? D : 1];
        const float* ktj = REG ? kt + (row0 + j) * ldt + h * dk : nullptr;
        if constexpr (D > 0 && REG) {
#pragma unroll
            for (int d = 0; d < D; d++) ktr[d] = ktj[d];
            ktj = ktr;
        }
        for (int i = 0; i < A; i++) {
            const float* qi = qs + i * KD + h * dk;
            const float* di = ds + i * VD + h * dv;
            const float* sp = st + (i * heads + h) * NS;
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < RD; d++)
                if (d < dk) s = fmaf(qi[d], kj[d], s);
#pragma unroll
            for (int d = 0; d < RD; d++)
                if (d < dv) dp = fmaf(di[d], vj[d], dp);
            s *= scale;
            const bool a = sadj[i * A + j] != 0;
            const float pij = expf((a ? s : -1e9f) - sp[0]) * sp[1];
            float dw = a ? pij * (dp - sp[2]) : 0.f;
            if (REG) {
                const float* qti = qts + i * KD + h * dk;
                float t = 0.f;
#pragma unroll
                for (int d = 0; d < RD; d++)
                    if (d < dk) t = fmaf(qti[d], ktj[d], t);
                dw += sp[7] * (expf(s - sp[3]) * sp[4] - expf(t * scale - sp[5]) * sp[6]);
            }
#pragma unroll
            for (int d = 0; d < RD; d++) {
                if (d < dk) ak[d] = fmaf(dw, qi[d], ak[d]);
                if (d < dv) av[d] = fmaf(pij, di[d], av[d]);
            }
        }
        float* ok = dkk + (row0 + j) * ldd + h * dk;
        float* ov = dvv + (row0 + j) * ldd + h * dv;
        const float* dj = ds + j * VD + h * dv;
#pragma unroll
        for (int d = 0; d < RD; d++) {
            if (d < dk) ok[d] = ak[d] * scale;
            if (d < dv) ov[d] = av[d] + dj[d];
        }
    }
}

// Forward value of DGN's attention regulariser (gm_agent_attention_kl) for one env per block:
//   kl_row[i] = sum_heads sum_j t_ij (log t_ij - log p_ij),  p = softmax_j(w_i.), t = softmax_j(w_tar,i.)
// (both unmasked), heads and j ascending. Both score rows are recomputed from the k / k_tar rows staged in LDS:
//   sum_j t_j (log t_j - log p_j) = sum_j e^{a_j} (a_j - b_j) / sum_j e^{a_j} + log sum_j e^{b_j} - log sum_j e^{a_j}
// with a = w_tar - max w_tar, b = w - max w.
template <int D>
__global__ __launch_bounds__(256) void k_agent_attention_kl(const float* __restrict__ q, const float* __restrict__ k,
                                                            long long ld, const float* __restrict__ qt,
                                                            const float* __restrict__ kt, long long ldt, int A,
                                                            int heads, int dk_, float scale,
                                                            float* __restrict__ kl_row) {
    constexpr int RD = D > 0 ? D : MAXD;
    const int dk = D > 0 ? D : dk_;
    extern __shared__ float sm[];
    const int b = blockIdx.x;
    const int KD = heads * dk;
    float* ks = sm;             // [A][KD]
    float* kts = ks + A * KD;   // [A][KD]
    float* klh = kts + A * KD;  // [A][heads]
    const long long row0 = (long long)b * A;
    for (int idx = threadIdx.x; idx < A * KD; idx += blockDim.x) {
        const int j = idx / KD, c = idx - j * KD;
        ks[idx] = k[(row0 + j) * ld + c];
        kts[idx] = kt[(row0 + j) * ldt + c];
    }
    __syncthreads();
    for (int p = threadIdx.x; p < A * heads; p += blockDim.x) {
        const int i = p / heads, h = p - i * heads;
        float qi[RD], qti[RD];
        const float* qr = q + (row0 + i) * ld + h * dk;
        const float* qtr = qt + (row0 + i) * ldt + h * dk;
#pragma unroll
        for (int d = 0; d < RD; d++)
            if (d < dk) {
                qi[d] = qr[d];
                qti[d] = qtr[d];
            }
        float mxu = -INFINITY, mxt = -INFINITY;
        for (int j = 0; j < A; j++) {
            const float* kj = ks + j * KD + h * dk;
            const float* ktj = kts + j * KD + h * dk;
            float s = 0.f, t = 0.f;
#pragma unroll
            for (int d = 0; d < RD; d++)
                if (d < dk) {
                    s = fmaf(qi[d], kj[d], s);
                    t = fmaf(qti[d], ktj[d], t);
                }
            mxu = fmaxf(mxu, s * scale);
            mxt = fmaxf(mxt, t * scale);
        }
        float su = 0.f, stt = 0.f, num = 0.f;
        for (int j = 0; j < A; j++) {
            const float* kj = ks + j * KD + h * dk;
            const float* ktj = kts + j * KD + h * dk;
            float s = 0.f, t = 0.f;
#pragma unroll
            for (int d = 0; d < RD; d++)
                if (d < dk) {
                    s = fmaf(qi[d], kj[d], s);
                    t = fmaf(qti[d], ktj[d], t);
                }
            const float bj = s * scale - mxu, aj = t * scale - mxt;
            const float ea = expf(aj);
            su += expf(bj);
            stt += ea;
            num = fmaf(ea, aj - bj, num);
        }
        klh[p] = num / stt + (logf(su) - logf(stt));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < A; i += blockDim.x) {
        float s = 0.f;
        for (int h = 0; h < heads; h++) s += klh[i * heads + h];
        kl_row[row0 + i] = s;
    }
}

int launched(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return gm_fail(GM_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return GM_OK;
}

}  // namespace

// Dynamic LDS above 64 KB has to be asked for per kernel before the launch; nothing to do at or below it.
template <typename K>
static bool lds_opt_in(K kern, size_t lds) {
    return lds <= 64 * 1024 ||
           hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
}

extern "C" int gm_agent_attention(const float* q, const float* k, const float* v, int64_t ld, const int8_t* adj,
                                  int32_t B, int32_t A, int32_t heads, int32_t dk, int32_t dv, float* out,
                                  int64_t ldo, float* att_weights, void* stream) {
    if (!q || !k || !v || !adj || !out || B <= 0 || A <= 0 || A > MAXA || heads <= 0 || dk <= 0 || dk > MAXD ||
        dv <= 0 || dv > MAXD || ld < (int64_t)heads * (dk > dv ? dk : dv) || ldo < (int64_t)heads * dv)
        return gm_fail(GM_ERR_INVALID_ARG, "gm_agent_attention: bad arguments (A <= 64, dk, dv <= 64)");
    const size_t lds = (size_t)A * heads * (dk + dv) * sizeof(float);
    if (lds > 160 * 1024) return gm_fail(GM_ERR_UNSUPPORTED, "gm_agent_attention: A * heads * (dk + dv) too large");
    const float scale = 1.0f / sqrtf((float)dk);
    if (dk == 16 && dv == 16) {
        if (!lds_opt_in(k_agent_attention<16>, lds)) return gm_fail(GM_ERR_HIP, "gm_agent_attention: LDS size refused");
        gm_set_last_kernel("k_agent_attention<16>");
        hipLaunchKernelGGL(k_agent_attention<16>, dim3(B), dim3(256), lds, (hipStream_t)stream, q, k, v,
                           (long long)ld, adj, A, heads, dk, dv, scale, out, (long long)ldo, att_weights);
    } else {
        if (!lds_opt_in(k_agent_attention<0>, lds)) return gm_fail(GM_ERR_HIP, "gm_agent_attention: LDS size refused");
        gm_set_last_kernel("k_agent_attention<0>");
        hipLaunchKernelGGL(k_agent_attention<0>, dim3(B), dim3(256), lds, (hipStream_t)stream, q, k, v,
                           (long long)ld, adj, A, heads, dk, dv, scale, out, (long long)ldo, att_weights);
    }
    return launched("gm_agent_attention");
}

extern "C" int gm_agent_comm(const float* h, int64_t ldh, const int8_t* adj, int32_t B, int32_t A, int32_t H,
                             float* out, int64_t ldo, void* stream) {
    if (!h || !adj || !out || B <= 0 || A <= 0 || A > MAXA || H <= 0 || ldh < H || ldo < H || h == out)
        return gm_fail(GM_ERR_INVALID_ARG, "gm_agent_comm: bad arguments (A <= 64, out must not alias h)");
    gm_set_last_kernel("k_agent_comm");
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
    if (H % 4 == 0 && a16(g0, ld0) && a16(g1, ld1) && a16(dh, ldd)) {
        gm_set_last_kernel("k_agent_comm_bwd<4>");
        hipLaunchKernelGGL(k_agent_comm_bwd<4>, grid, dim3(256), 0, (hipStream_t)stream, g0, (long long)ld0, g1,
                           (long long)ld1, adj, A, H, dh, (long long)ldd);
    } else {
        gm_set_last_kernel("k_agent_comm_bwd<1>");
        hipLaunchKernelGGL(k_agent_comm_bwd<1>, grid, dim3(256), 0, (hipStream_t)stream, g0, (long long)ld0, g1,
                           (long long)ld1, adj, A, H, dh, (long long)ldd);
    }
    return launched("gm_agent_comm_bwd");
}

// LDS bytes of k_agent_attention_bwd: the k, v (and k_tar) rows, then q, dout (q_tar) over them; the row statistics, adj
static size_t attention_bwd_lds(int A, int heads, int dk, int dv, bool reg) {
    const size_t fl = (size_t)A * heads * ((reg ? 2 : 1) * (size_t)dk + (size_t)dv + (reg ? 8 : 3));
    return fl * sizeof(float) + (((size_t)A * A + 15) & ~(size_t)15);
}

extern "C" int gm_agent_attention_bwd(const float* q, const float* k, const float* v, int64_t ld, const int8_t* adj,
                                      int32_t B, int32_t A, int32_t heads, int32_t dk, int32_t dv, const float* dout,
                                      int64_t ldo, const float* q_tar, const float* k_tar, int64_t ld_tar,
                                      const float* r, float* dq, float* dk_out, float* dv_out, int64_t ldd,
                                      void* stream) {
    const bool reg = q_tar != nullptr;
    if (!q || !k || !v || !adj || !dout || !dq || !dk_out || !dv_out || B <= 0 || A <= 0 || A > MAXA || heads <= 0 ||
        dk <= 0 || dk > MAXD || dv <= 0 || dv > MAXD || ld < (int64_t)heads * (dk > dv ? dk : dv) ||
        ldo < (int64_t)heads * dv || ldd < (int64_t)heads * (dk > dv ? dk : dv) || (q_tar == nullptr) != (k_tar == nullptr) ||
        (reg && ld_tar < (int64_t)heads * dk) || (r && !reg))
        return gm_fail(GM_ERR_INVALID_ARG,
                       "gm_agent_attention_bwd: bad arguments (A <= 64, dk, dv <= 64; q_tar and k_tar together, r "
                       "only with them)");
    const size_t lds = attention_bwd_lds(A, heads, dk, dv, reg);
    if (lds > 160 * 1024)
        return gm_fail(GM_ERR_UNSUPPORTED, "gm_agent_attention_bwd: the env's rows need more than 160 KB of LDS");
    const float scale = 1.0f / sqrtf((float)dk);
#define GM_ATT_BWD(DD, RR)                                                                                          \
    do {                                                                                                            \
        if (!lds_opt_in(k_agent_attention_bwd<DD, RR>, lds))                                                        \
            return gm_fail(GM_ERR_HIP, "gm_agent_attention_bwd: LDS size refused");                                 \
        gm_set_last_kernel((RR) ? "k_agent_attention_bwd<" #DD ",reg>" : "k_agent_attention_bwd<" #DD ",plain>");   \
        hipLaunchKernelGGL((k_agent_attention_bwd<DD, RR>), dim3(B), dim3(256), lds, (hipStream_t)stream, q, k, v,  \
                           (long long)ld, adj, A, heads, dk, dv, scale, dout, (long long)ldo, q_tar, k_tar,         \
                           (long long)ld_tar, r, dq, dk_out, dv_out, (long long)ldd);                               \
    } while (0)
    const bool d16 = dk == 16 && dv == 16;
    if (d16 && reg) GM_ATT_BWD(16, true);
    else if (d16) GM_ATT_BWD(16, false);
    else if (reg) GM_ATT_BWD(0, true);
    else GM_ATT_BWD(0, false);
#undef GM_ATT_BWD
    return launched("gm_agent_attention_bwd");
}

extern "C" int gm_agent_attention_kl(const float* q, const float* k, int64_t ld, const float* q_tar,
                                     const float* k_tar, int64_t ld_tar, int32_t B, int32_t A, int32_t heads,
                                     int32_t dk, float* kl_row, void* stream) {
    if (!q || !k || !q_tar || !k_tar || !kl_row || B <= 0 || A <= 0 || A > MAXA || heads <= 0 || dk <= 0 ||
        dk > MAXD || ld < (int64_t)heads * dk || ld_tar < (int64_t)heads * dk)
        return gm_fail(GM_ERR_INVALID_ARG, "gm_agent_attention_kl: bad arguments (A <= 64, dk <= 64)");
    const size_t lds = (size_t)A * heads * (2 * (size_t)dk + 1) * sizeof(float);
    if (lds > 160 * 1024)
        return gm_fail(GM_ERR_UNSUPPORTED, "gm_agent_attention_kl: the env's rows need more than 160 KB of LDS");
    const float scale = 1.0f / sqrtf((float)dk);
    if (dk == 16) {
        if (!lds_opt_in(k_agent_attention_kl<16>, lds)) return gm_fail(GM_ERR_HIP, "gm_agent_attention_kl: LDS size refused");
        gm_set_last_kernel("k_agent_attention_kl<16>");
        hipLaunchKernelGGL(k_agent_attention_kl<16>, dim3(B), dim3(256), lds, (hipStream_t)stream, q, k, (long long)ld,
                           q_tar, k_tar, (long long)ld_tar, A, heads, dk, scale, kl_row);
    } else {
        if (!lds_opt_in(k_agent_attention_kl<0>, lds)) return gm_fail(GM_ERR_HIP, "gm_agent_attention_kl: LDS size refused");
        gm_set_last_kernel("k_agent_attention_kl<0>");
        hipLaunchKernelGGL(k_agent_attention_kl<0>, dim3(B), dim3(256), lds, (hipStream_t)stream, q, k, (long long)ld,
                           q_tar, k_tar, (long long)ld_tar, A, heads, dk, scale, kl_row);
    }
    return launched("gm_agent_attention_kl");
}
