// gm_netmon.hip — NetMon message passing (reference src/model.py:206-229,
// 476-631) as HBM-bound HIP kernels for gfx950.
//
// Graph layout: node rows h[G*N][H] (fp32, row-major; float4 lanes when H % 4 == 0), neighbour
// table nbr[G][N][deg] (ELL, ascending ids, -1 = none). The reference multiplies a
// dense (I+A) mask with h (bmm); with deg 3 that reads 4 rows per output row, so
// the aggregate is a gather of 4 contiguous 512-byte rows per node with float4
// lanes: 32 lanes per row, a wave covers 2 rows, consecutive rows share the same
// graph's 10 KB working set in L2.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/graph_marl_amd.h"
#include "../../include/graph_marl_amd_tuning.h"
#include "gm_amax.hpp"
#include "gm_act.hpp"
#include "gm_device.hpp"

int gm_fail(int code, const std::string& msg);

namespace {

constexpr int MAXDEG = 8;

// V-wide fp32 vectors (V = 4, 2 or 1 chosen from H's alignment on the host)
template <int V> struct Vec { float v[V]; };
template <int V> __device__ __forceinline__ Vec<V> ldv(const float* p) {
    Vec<V> r;
    if constexpr (V == 4) {
        float4 t = *reinterpret_cast<const float4*>(p);
        r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
    } else if constexpr (V == 2) {
        float2 t = *reinterpret_cast<const float2*>(p);
        r.v[0] = t.x; r.v[1] = t.y;
    } else {
        r.v[0] = *p;
    }
    return r;
}
template <int V> __device__ __forceinline__ void stv(float* p, const Vec<V>& a) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(a.v[0], a.v[1], a.v[2], a.v[3]);
    else if constexpr (V == 2) *reinterpret_cast<float2*>(p) = make_float2(a.v[0], a.v[1]);
    else *p = a.v[0];
}
template <int V> __device__ __forceinline__ Vec<V> zerov() {
    Vec<V> r;
#pragma unroll
    for (int i = 0; i < V; i++) r.v[i] = 0.f;
    return r;
}

// sorted member list {n} ∪ nbr(n) (ascending node id) — the summation order of a
// sequential dense row product (I+A)[n,:] · h
__device__ __forceinline__ int members(const int32_t* nb, int deg, int n, int* out) {
    int cnt = 0;
    bool self_done = false;
    for (int k = 0; k < deg; k++) {
        int v = nb[k];
        if (v < 0) continue;
        if (!self_done && n < v) {
            out[cnt++] = n;
            self_done = true;
        }
        out[cnt++] = v;
    }
    if (!self_done) out[cnt++] = n;
    return cnt;
}

__device__ __forceinline__ float4 f4add(float4 a, float4 b) {
    return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

// XCD-aware block order: the hardware deals block b to XCD b % 8; logical block numbers are
// handed out so that each XCD gets one contiguous run of rows, and the 4 rows every node reads
// (itself + 3 neighbours of the same graph) sit in that XCD's L2 instead of being fetched once per
// XCD that touches the graph (a graph's 20 rows span 3 consecutive 8-row blocks)
__device__ __forceinline__ unsigned xcd_block(unsigned bid, unsigned T) {
    const unsigned q = T / 8, r = T % 8, x = bid % 8, loc = bid / 8;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + loc;
}

// forward: out[n] = Σ_{m ∈ {n} ∪ nbr(n)} h[m]  (/ count for mean)
// backward (symmetric adjacency): dh[j] = Σ_{n ∈ {j} ∪ nbr(j)} dout[n] * scale(n)
template <bool BWD, int V>
__global__ __launch_bounds__(256) void k_mp_aggregate(const float* __restrict__ h, const int32_t* __restrict__ nbr,
                                                      int G, int N, int deg, int H, int mode, float* __restrict__ out,
                                                      long long ldh, long long ldo) {
    const int HV = H / V;
    const long long gid = (long long)xcd_block(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
    const long long total = (long long)G * N * HV;
    if (gid >= total) return;
    const int cv = (int)(gid % HV);
    const long long row = gid / HV;
    const int g = (int)(row / N), n = (int)(row % N);
    const int32_t* nb = nbr + ((size_t)g * N + n) * deg;
    int mem[MAXDEG + 1];
    const int cnt = members(nb, deg, n, mem);
    const float* src = h + (size_t)g * N * ldh + (size_t)cv * V;
    Vec<V> acc = zerov<V>();
    if (!BWD && deg <= 3) {
        // routing graphs (degree 3): the up to 4 member rows are loaded back to back (independent
        // loads in flight together), then summed in ascending id order like the general loop
        Vec<V> x[4];
#pragma unroll
        for (int q = 0; q < 4; q++) x[q] = q < cnt ? ldv<V>(src + (size_t)mem[q] * ldh) : zerov<V>();
        acc = x[0];
#pragma unroll
        for (int q = 1; q < 4; q++)
            if (q < cnt) {
#pragma unroll
                for (int i = 0; i < V; i++) acc.v[i] = acc.v[i] + x[q].v[i];
            }
        if (mode == 1) {
#pragma unroll
            for (int i = 0; i < V; i++) acc.v[i] = acc.v[i] / cnt;
        }
        stv<V>(out + row * ldo + (size_t)cv * V, acc);
        return;
    }
    for (int q = 0; q < cnt; q++) {
        Vec<V> x = ldv<V>(src + (size_t)mem[q] * ldh);
        if (BWD && mode == 1) {
            const int32_t* nbm = nbr + ((size_t)g * N + mem[q]) * deg;
            int cm = 1;
            for (int k = 0; k < deg; k++) cm += nbm[k] >= 0;
#pragma unroll
            for (int i = 0; i < V; i++) x.v[i] = x.v[i] * (1.0f / (float)cm);
        }
#pragma unroll
        for (int i = 0; i < V; i++) acc.v[i] = q == 0 ? x.v[i] : acc.v[i] + x.v[i];
    }
    if (!BWD && mode == 1) {
#pragma unroll
        for (int i = 0; i < V; i++) acc.v[i] = acc.v[i] / cnt;
    }
    stv<V>(out + row * ldo + (size_t)cv * V, acc);
}

// forward of k_mp_aggregate for degree-3 graphs with fewer than 2^31 (row, vector) items: 32-bit index
// math (the 64-bit divisions of the general kernel were most of its instructions) and the members
// {n} u nbr(n) put in ascending id order by a 4-input sorting network (missing neighbours last) instead of
// members()'s dynamically indexed local array; the same members, the same summation order
template <int V>
__global__ __launch_bounds__(256) void k_mp_aggregate3(const float* __restrict__ h, const int32_t* __restrict__ nbr,
                                                       unsigned N, unsigned HV, int mode, float* __restrict__ out,
                                                       long long ldh, long long ldo, unsigned total) {
    const unsigned gid = xcd_block(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const unsigned row = gid / HV, cv = gid - row * HV;
    const unsigned g = row / N;
    const int32_t* nb = nbr + (size_t)row * 3;
    constexpr int MISSING = 0x7fffffff;
    int m[4] = {(int)(row - g * N), nb[0] < 0 ? MISSING : nb[0], nb[1] < 0 ? MISSING : nb[1],
                nb[2] < 0 ? MISSING : nb[2]};
    const int cnt = 1 + (m[1] != MISSING) + (m[2] != MISSING) + (m[3] != MISSING);
    auto cswap = [](int& a, int& b) {
        const int lo = min(a, b), hi = max(a, b);
        a = lo;
        b = hi;
    };
    cswap(m[0], m[1]);
    cswap(m[2], m[3]);
    cswap(m[0], m[2]);
    cswap(m[1], m[3]);
    cswap(m[1], m[2]);
    const float* src = h + (size_t)g * N * ldh + (size_t)cv * V;
    Vec<V> x[4];
#pragma unroll
    for (int q = 0; q < 4; q++) x[q] = q < cnt ? ldv<V>(src + (size_t)m[q] * ldh) : zerov<V>();
    Vec<V> acc = x[0];
#pragma unroll
    for (int q = 1; q < 4; q++)
        if (q < cnt) {
#pragma unroll
            for (int i = 0; i < V; i++) acc.v[i] = acc.v[i] + x[q].v[i];
        }
    if (mode == 1) {
#pragma unroll
        for (int i = 0; i < V; i++) acc.v[i] = acc.v[i] / cnt;
    }
    stv<V>(out + (size_t)row * ldo + (size_t)cv * V, acc);
}

// K rounds of the aggregate (stateless NetMon, src/model.py:509-554 with rnn_type "none": h = M) with the
// graphs of a block resident in LDS: two [rows, P] fp32 images (P = row pitch in floats, H or H + 4 so that
// the 16-byte reads of rows of equal parity do not all start on one bank), read once from HBM, ping-ponged
// K times, and only h_K (and h_{K-1}, the reference's last_neighbor_h) written back. The pad's effect on the
// round time has not been measured (at H >= 256 a wave reads one row, so no two rows meet in a lane group).
// A block holds gpb whole graphs; thread t owns 16-byte lane t % HV of rows t / HV, t / HV + blockDim / HV, .. (blockDim is a
// multiple of HV: no division inside the rounds). The sorted member lists {n} u nbr(n) are built once per
// block into LDS as block-local row numbers. Every round does the arithmetic of one k_mp_aggregate launch:
// forward the members summed in ascending id order, then / count for mean; backward every member scaled by
// 1 / count(member) for mean, product and sum rounded separately, summed in the same order
// (bit-identical to the chained launches, tests/test_stateless_gpu.py).
// BWD: round 0 also adds `add` (the gradient of h_{K-1}), rounded after the sum like a separate add.
template <bool BWD>
__global__ __launch_bounds__(1024) void k_mp_iterate(const float* __restrict__ src, long long lds,
                                                     const float* __restrict__ add, long long lda,
                                                     const int32_t* __restrict__ nbr, int G, int N, int deg, int H,
                                                     int P, int gpb, int mode, int iters, float* __restrict__ out,
                                                     long long ldo, float* __restrict__ prev, long long ldp) {
    extern __shared__ __attribute__((aligned(16))) float smi[];
    const int g0 = blockIdx.x * gpb;
    const int rows = min(gpb, G - g0) * N, cap = gpb * N;
    float* cur = smi;
    float* nxt = smi + (size_t)cap * P;
    int* mlist = reinterpret_cast<int*>(nxt + (size_t)cap * P);  // [cap][deg + 1]
    int* mcnt = mlist + (size_t)cap * (deg + 1);                 // [cap]
    float* mscale = reinterpret_cast<float*>(mcnt + cap);        // [cap] (BWD, mean)
    const int HV = H >> 2, D1 = deg + 1;
    const int cv4 = ((int)threadIdx.x % HV) * 4, r0 = (int)threadIdx.x / HV, rstep = (int)blockDim.x / HV;
    const size_t grow0 = (size_t)g0 * N;
    for (int lr = threadIdx.x; lr < rows; lr += blockDim.x) {
        const int n = lr % N, base = lr - n;
        int mem[MAXDEG + 1];
        const int cnt = members(nbr + (grow0 + lr) * deg, deg, n, mem);
        for (int q = 0; q < cnt; q++) mlist[lr * D1 + q] = base + mem[q];
        mcnt[lr] = cnt;
        if (BWD) mscale[lr] = 1.0f / (float)cnt;
    }
    for (int lr = r0; lr < rows; lr += rstep)
        *reinterpret_cast<float4*>(cur + (size_t)lr * P + cv4) =
            *reinterpret_cast<const float4*>(src + (grow0 + lr) * lds + cv4);
    __syncthreads();
    for (int it = 0; it < iters; it++) {
        for (int lr = r0; lr < rows; lr += rstep) {
            const int cnt = mcnt[lr];
            const int* ml = mlist + lr * D1;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            if (!BWD) {
                acc = *reinterpret_cast<const float4*>(cur + (size_t)ml[0] * P + cv4);
                for (int q = 1; q < cnt; q++) acc = f4add(acc, *reinterpret_cast<const float4*>(cur + (size_t)ml[q] * P + cv4));
                if (mode == 1) {
                    acc.x = acc.x / cnt;
                    acc.y = acc.y / cnt;
                    acc.z = acc.z / cnt;
                    acc.w = acc.w / cnt;
                }
            } else {
                for (int q = 0; q < cnt; q++) {
                    const int m = ml[q];
                    float4 x = *reinterpret_cast<const float4*>(cur + (size_t)m * P + cv4);
                    if (mode == 1) {
                        const float s = mscale[m];
                        x = make_float4(__fmul_rn(x.x, s), __fmul_rn(x.y, s), __fmul_rn(x.z, s), __fmul_rn(x.w, s));
                    }
                    acc = q == 0 ? x
                                 : make_float4(__fadd_rn(acc.x, x.x), __fadd_rn(acc.y, x.y), __fadd_rn(acc.z, x.z),
                                               __fadd_rn(acc.w, x.w));
                }
                if (it == 0 && add) {
                    const float4 a = *reinterpret_cast<const float4*>(add + (grow0 + lr) * lda + cv4);
                    acc = make_float4(__fadd_rn(acc.x, a.x), __fadd_rn(acc.y, a.y), __fadd_rn(acc.z, a.z),
                                      __fadd_rn(acc.w, a.w));
                }
            }
            *reinterpret_cast<float4*>(nxt + (size_t)lr * P + cv4) = acc;
        }
        __syncthreads();
        float* t = cur;
        cur = nxt;
        nxt = t;
    }
    for (int lr = r0; lr < rows; lr += rstep) {
        *reinterpret_cast<float4*>(out + (grow0 + lr) * ldo + cv4) =
            *reinterpret_cast<const float4*>(cur + (size_t)lr * P + cv4);
        if (!BWD)
            *reinterpret_cast<float4*>(prev + (grow0 + lr) * ldp + cv4) =
                *reinterpret_cast<const float4*>(nxt + (size_t)lr * P + cv4);
    }
}

// the chained form's pieces: out = h0 and prev = 0 (K = 0), and x += y over strided rows (the backward's add)
template <int V>
__global__ __launch_bounds__(256) void k_mp_copy_rows(const float* __restrict__ h, long long ldh, long long rows,
                                                      int HV, float* __restrict__ out, long long ldo,
                                                      float* __restrict__ prev, long long ldp) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= rows * HV) return;
    const long long row = gid / HV;
    const int c = (int)(gid - row * HV) * V;
    stv<V>(out + row * ldo + c, ldv<V>(h + row * ldh + c));
    if (prev) stv<V>(prev + row * ldp + c, zerov<V>());
}

template <int V>
__global__ __launch_bounds__(256) void k_mp_add_rows(float* __restrict__ x, long long ldx, const float* __restrict__ y,
                                                     long long ldy, long long rows, int HV) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= rows * HV) return;
    const long long row = gid / HV;
    const int c = (int)(gid - row * HV) * V;
    Vec<V> a = ldv<V>(x + row * ldx + c);
    const Vec<V> b = ldv<V>(y + row * ldy + c);
#pragma unroll
    for (int i = 0; i < V; i++) a.v[i] = a.v[i] + b.v[i];
    stv<V>(x + row * ldx + c, a);
}

// readout: out row r of graph g = [h_final[v], h_prev[nbr(v,0..deg-1)]], v = agent_node or r.
// Output rows may sit inside a wider joint observation (stride); V-wide stores.
template <int V>
__global__ __launch_bounds__(256) void k_readout(const float* __restrict__ hf, const float* __restrict__ hp,
                                                 const int32_t* __restrict__ nbr, const int32_t* __restrict__ agent_node,
                                                 int G, int N, int R, int deg, int H, float* __restrict__ out,
                                                 long long stride, long long ldf, long long ldp) {
    const int HV = H / V;
    const int WV = (deg + 1) * HV;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)G * R * WV;
    if (gid >= total) return;
    const int cv = (int)(gid % WV);
    const long long row = gid / WV;
    const int g = (int)(row / R), r = (int)(row % R);
    const int v = agent_node ? agent_node[(size_t)g * R + r] : r;
    const int seg = cv / HV, off = (cv - seg * HV) * V;
    Vec<V> val;
    if (seg == 0) {
        val = ldv<V>(hf + ((size_t)g * N + v) * ldf + off);
    } else {
        int m = nbr[((size_t)g * N + v) * deg + seg - 1];
        val = m >= 0 ? ldv<V>(hp + ((size_t)g * N + m) * ldp + off) : zerov<V>();
    }
    stv<V>(out + row * stride + (size_t)cv * V, val);
}

// readout backward, deterministic (no atomics): node v of graph g gathers the
// gradient of every row that read it, rows in ascending order.
template <int V>
__global__ __launch_bounds__(256) void k_readout_bwd(const float* __restrict__ dout, long long stride,
                                                     const int32_t* __restrict__ nbr,
                                                     const int32_t* __restrict__ agent_node, int G, int N, int R,
                                                     int deg, int H, float* __restrict__ dhf, float* __restrict__ dhp) {
    const int HV = H / V;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)G * N * HV;
    if (gid >= total) return;
    const int off = (int)(gid % HV) * V;
    const long long node = gid / HV;
    const int g = (int)(node / N), v = (int)(node % N);
    Vec<V> af = zerov<V>(), ap = zerov<V>();
    for (int r = 0; r < R; r++) {
        const int u = agent_node ? agent_node[(size_t)g * R + r] : r;
        const float* drow = dout + ((size_t)g * R + r) * stride;
        if (u == v) {
            Vec<V> x = ldv<V>(drow + off);
#pragma unroll
            for (int i = 0; i < V; i++) af.v[i] += x.v[i];
        }
        const int32_t* nb = nbr + ((size_t)g * N + u) * deg;
        for (int k = 0; k < deg; k++) {
            if (nb[k] == v) {
                Vec<V> x = ldv<V>(drow + (size_t)(k + 1) * H + off);
#pragma unroll
                for (int i = 0; i < V; i++) ap.v[i] += x.v[i];
            }
        }
    }
    if (dhf) stv<V>(dhf + node * H + off, af);
    if (dhp) stv<V>(dhp + node * H + off, ap);
}

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// nn.LSTMCell gate math (i, f, g, o): c' = σ(f)c + σ(i)tanh(g), h' = σ(o)tanh(c')
__global__ __launch_bounds__(256) void k_lstm_pw(const float* __restrict__ gates, const float* __restrict__ c,
                                                 int M, int H, float* __restrict__ h1, float* __restrict__ c1,
                                                 float* __restrict__ act) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)M * H) return;
    const long long m = gid / H;
    const int j = (int)(gid % H);
    const float* g = gates + m * 4 * H;
    float i = sigm(g[j]), f = sigm(g[H + j]), gg = tanhf(g[2 * H + j]), o = sigm(g[3 * H + j]);
    float cn = f * c[gid] + i * gg;
    float hn = o * tanhf(cn);
    c1[gid] = cn;
    h1[gid] = hn;
    if (act) {
        float* a = act + m * 4 * H;
        a[j] = i;
        a[H + j] = f;
        a[2 * H + j] = gg;
        a[3 * H + j] = o;
    }
}

__global__ __launch_bounds__(256) void k_lstm_pw_bwd(const float* __restrict__ dh1, const float* __restrict__ dc1,
                                                     const float* __restrict__ act, const float* __restrict__ c,
                                                     const float* __restrict__ c1, int M, int H,
                                                     float* __restrict__ dgates, float* __restrict__ dc,
                                                     unsigned* __restrict__ amax) {
    float mx = 0.f;
    const long long total = (long long)M * H;
    for (long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x; gid < total;
         gid += (long long)gridDim.x * blockDim.x) {
        const long long m = gid / H;
        const int j = (int)(gid % H);
        const float* a = act + m * 4 * H;
        float i = a[j], f = a[H + j], gg = a[2 * H + j], o = a[3 * H + j];
        float tc = tanhf(c1[gid]);
        float dh = dh1 ? dh1[gid] : 0.f;
        float dct = (dc1 ? dc1[gid] : 0.f) + dh * o * (1.f - tc * tc);
        float* dg = dgates + m * 4 * H;
        const float d0 = dct * gg * i * (1.f - i), d1 = dct * c[gid] * f * (1.f - f);
        const float d2 = dct * i * (1.f - gg * gg), d3 = dh * tc * o * (1.f - o);
        dg[j] = d0;
        dg[H + j] = d1;
        dg[2 * H + j] = d2;
        dg[3 * H + j] = d3;
        dc[gid] = dct * f;
        mx = fmaxf(mx, fmaxf(fmaxf(fabsf(d0), fabsf(d1)), fmaxf(fabsf(d2), fabsf(d3))));
    }
    if (amax) gm_block_amax(amax, mx);
}


// bits 0..15 of x to the even bit positions 0, 2, .., 30
__device__ __forceinline__ unsigned spread16(unsigned x) {
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}

// First NetMon encoder layer on routing node observations (src/model.py:272-276 on the
// node obs of src/env/routing.py:187-235). Row n of graph g is
//   [onehot(n) | cnt | load | 3 x (onehot(nbr_k) | len_k | load_k)]
// so W x touches 12 of the 4N+8 weight columns: the dense GEMM's K = 4N+8 collapses to a
// 12-term gather over W^T staged in LDS (BN output columns per block, 64 lanes x BN/64
// columns). HBM-bound on the output rows (n floats per node).
template <int AC>
__device__ __forceinline__ float renc_act(float v, int act) {
    if constexpr (AC == 0)
        return v;
    else if constexpr (AC == 1)
        return v >= 0.f ? v : 0.01f * v;
    else
        return gm_act_fast(v, act);
}

// AC: the activation at compile time (0 none, 1 leaky_relu) or -1 = GM_ACT_* `act` at run time (a per
// element branch tree: kept out of the default kernels, it cost 65 -> 76 us per 81 920 rows)
template <int CPL, int AC, int TPB = 256>  // output columns per lane (BN = 64 * CPL), threads per block
__global__ __launch_bounds__(TPB) void k_routing_enc(const float* __restrict__ x, long long ldx,
                                                     const int32_t* __restrict__ nbr, int G, int N,
                                                     const float* __restrict__ wt, const float* __restrict__ b,
                                                     int n, int act, float* __restrict__ y, long long ldy,
                                                     int rows_per_block, unsigned* __restrict__ sbits,
                                                     long long ldsb) {
    constexpr int BN = 64 * CPL;
    extern __shared__ __attribute__((aligned(16))) float sw[];  // [K][BN]
    const int K = 4 * N + 8;
    const int c0 = blockIdx.y * BN;
    for (int i = threadIdx.x; i < K * (BN / 4); i += blockDim.x) {
        const int r = i / (BN / 4), c4 = i - r * (BN / 4);
        reinterpret_cast<float4*>(sw)[i] = *reinterpret_cast<const float4*>(wt + (size_t)r * n + c0 + 4 * c4);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = CPL * lane;
    float bias[CPL];
#pragma unroll
    for (int j = 0; j < CPL; j++) bias[j] = b ? b[c0 + col + j] : 0.f;
    const long long M = (long long)G * N;
    // each wave owns groups of 64 consecutive rows: lane l gathers the 11 nonzero features of
    // row base + l up front (coalesced, one latency), the row loop broadcasts them by readlane;
    // the block's W^T slice is staged once for rows_per_block rows
    const long long bend = min(M, (long long)(blockIdx.x + 1) * rows_per_block);
    for (long long base = (long long)blockIdx.x * rows_per_block + (long long)wv * 64; base < bend;
         base += (blockDim.x >> 6) * 64) {
    const int nrows = bend - base < 64 ? (int)(bend - base) : 64;
    int fv = 0, f_nb[3] = {0, 0, 0};
    float f_cnt = 0.f, f_tl = 0.f, f_len[3] = {0.f, 0.f, 0.f}, f_ld[3] = {0.f, 0.f, 0.f};
    if (lane < nrows) {
        const long long r = base + lane;
        const int g = (int)(r / N);
        fv = (int)(r - (long long)g * N);
        const float* xr = x + r * ldx;
        f_cnt = xr[N];
        f_tl = xr[N + 1];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int off = N + 2 + k * (N + 2);
            f_len[k] = xr[off + N];
            f_ld[k] = xr[off + N + 1];
            f_nb[k] = nbr[((size_t)g * N + fv) * 3 + k];
        }
    }
    // weight columns of the 8 scalar features (cnt, load, 3 x (len, load)) stay in registers;
    // only the 4 one-hot columns (node, 3 neighbours) are looked up in LDS per row
    float wc[4][2][CPL];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int off = k == 0 ? N : N + 2 + (k - 1) * (N + 2) + N;
#pragma unroll
        for (int j = 0; j < CPL; j++) {
            wc[k][0][j] = sw[off * BN + col + j];
            wc[k][1][j] = sw[(off + 1) * BN + col + j];
        }
    }
    for (int i = 0; i < nrows; i++) {
        const int v = __builtin_amdgcn_readlane(fv, i);
        const float cnt = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(f_cnt), i));
        const float tl = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(f_tl), i));
        float acc[CPL];
        // one-hot weight rows as 8-byte LDS reads (CPL = 2: ds_read_b64 is conflict-free; the
        // ds_read2_b32 the compiler made of two float reads spent 54 % of its LDS cycles in bank
        // conflicts, though the kernel time did not change: 57.5 vs 57.7 us per 81 920 rows)
        auto wrow = [&](int r, float (&e)[CPL]) {
            if constexpr (CPL == 2) {
                const float2 t = *reinterpret_cast<const float2*>(sw + r * BN + col);
                e[0] = t.x;
                e[CPL - 1] = t.y;
            } else {
#pragma unroll
                for (int j = 0; j < CPL; j++) e[j] = sw[r * BN + col + j];
            }
        };
        float e0[CPL];
        wrow(v, e0);
#pragma unroll
        for (int j = 0; j < CPL; j++) acc[j] = bias[j] + e0[j] + cnt * wc[0][0][j] + tl * wc[0][1][j];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int off = N + 2 + k * (N + 2);
            const int u = __builtin_amdgcn_readlane(f_nb[k], i);
            const float ln = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(f_len[k]), i));
            const float ld = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(f_ld[k]), i));
            float ek[CPL];
            wrow(off + u, ek);
#pragma unroll
            for (int j = 0; j < CPL; j++) acc[j] += ek[j] + ln * wc[k + 1][0][j] + ld * wc[k + 1][1][j];
        }
        float* yr = y + (base + i) * ldy + c0 + col;
        if (CPL == 2) {
            float a0 = acc[0], a1 = acc[CPL - 1];
            a0 = renc_act<AC>(a0, act);
            a1 = renc_act<AC>(a1, act);
            *reinterpret_cast<float2*>(yr) = make_float2(a0, a1);
            if (sbits) {  // 32-column sign words: lanes 16k..16k+15 hold columns 32k..32k+31, two each
                const unsigned long long b0 = __ballot(a0 > 0.f), b1 = __ballot(a1 > 0.f);
                if ((lane & 15) == 0) {
                    const int k = lane >> 4;
                    sbits[(base + i) * ldsb + (c0 >> 5) + k] =
                        spread16((unsigned)(b0 >> (16 * k)) & 0xFFFFu) | (spread16((unsigned)(b1 >> (16 * k)) & 0xFFFFu) << 1);
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < CPL; j++) yr[j] = renc_act<AC>(acc[j], act);
            if (sbits) {
                const float a0 = renc_act<AC>(acc[0], act);
                const unsigned long long b0 = __ballot(a0 > 0.f);
                if ((lane & 31) == 0) sbits[(base + i) * ldsb + (c0 >> 5) + (lane >> 5)] = (unsigned)(b0 >> lane);
            }
        }
    }
    }
}

inline unsigned nblocks(long long total, int bs) { return (unsigned)((total + bs - 1) / bs); }

int launched() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return gm_fail(GM_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return GM_OK;
}

}  // namespace

// widest vector that divides H and keeps every access aligned (base pointers are
// torch allocations; strides are checked)
static int vec_width(int H, long long stride, const void* p) {
    if (H % 4 == 0 && stride % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) return 4;
    if (H % 2 == 0 && stride % 2 == 0 && (reinterpret_cast<uintptr_t>(p) & 7) == 0) return 2;
    return 1;
}

// gm_last_kernel (diagnostics, graph_marl_amd_tuning.h): every launch site of the dispatchers below names its
// kernel first: one host store per call. The state sits behind gm_set_last_kernel (gm_device.hpp), which the
// GEMM launchers of gm_gemm.hip call too.
static thread_local const char* g_last_kernel = "";
void gm_set_last_kernel(const char* name) { g_last_kernel = name; }
#define GM_RAN(NAME) gm_set_last_kernel(NAME)
extern "C" const char* gm_last_kernel(void) { return g_last_kernel; }
// gm_last_lnlstm_pw: the LayerNorm-LSTM forward names its kernel in a slot of its own. The recorded launch lists of
// the sequence-batched update (tests/golden/*_trace.json) read gm_last_kernel after every library call, this
// forward among them, and hold the name the call before it left there.
static thread_local const char* g_last_lnlstm_pw = "";
extern "C" const char* gm_last_lnlstm_pw(void) { return g_last_lnlstm_pw; }

#define GM_VLAUNCH(KER, V, GRID, ...)                                                                  \
    do {                                                                                               \
        GM_RAN((V) == 4 ? #KER "<4>" : (V) == 2 ? #KER "<2>" : #KER "<1>");                           \
        if ((V) == 4) hipLaunchKernelGGL(KER<4>, GRID, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); \
        else if ((V) == 2) hipLaunchKernelGGL(KER<2>, GRID, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); \
        else hipLaunchKernelGGL(KER<1>, GRID, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__);        \
    } while (0)

template <bool BWD>
static int launch_agg(const float* h, const int32_t* nbr, int32_t G, int32_t N, int32_t deg, int32_t H, int32_t mode,
                      float* out, void* stream, long long ldh = 0, long long ldo = 0) {
    if (!ldh) ldh = H;
    if (!ldo) ldo = H;
    const int V = vec_width(H, ldh, h) < vec_width(H, ldo, out) ? vec_width(H, ldh, h) : vec_width(H, ldo, out);
    long long total = (long long)G * N * (H / V);
    dim3 grid(nblocks(total, 256));
    if (!BWD && deg == 3 && total < (1ll << 31)) {
        GM_VLAUNCH(k_mp_aggregate3, V, grid, h, nbr, (unsigned)N, (unsigned)(H / V), mode, out, ldh, ldo, (unsigned)total);
        return launched();
    }
    if (BWD) GM_RAN(V == 4 ? "k_mp_aggregate<bwd,4>" : V == 2 ? "k_mp_aggregate<bwd,2>" : "k_mp_aggregate<bwd,1>");
    else GM_RAN(V == 4 ? "k_mp_aggregate<fwd,4>" : V == 2 ? "k_mp_aggregate<fwd,2>" : "k_mp_aggregate<fwd,1>");
    if (V == 4) hipLaunchKernelGGL((k_mp_aggregate<BWD, 4>), grid, dim3(256), 0, (hipStream_t)stream, h, nbr, G, N, deg, H, mode, out, ldh, ldo);
    else if (V == 2) hipLaunchKernelGGL((k_mp_aggregate<BWD, 2>), grid, dim3(256), 0, (hipStream_t)stream, h, nbr, G, N, deg, H, mode, out, ldh, ldo);
    else hipLaunchKernelGGL((k_mp_aggregate<BWD, 1>), grid, dim3(256), 0, (hipStream_t)stream, h, nbr, G, N, deg, H, mode, out, ldh, ldo);
    return launched();
}

// Backward of act(x W^T + b) with leaky_relu(0.01) after the Linear (reference MLP,
// src/model.py:13-42): g = dY * (Y >= 0 ? 1 : slope), and per-block column sums of g for the
// bias gradient (partial[block][col]; the caller sums the blocks: a fixed summation order).
// Threads own columns, blocks own row chunks; loads and stores are row-contiguous.
// act < 0: leaky_relu with the given slope; else GM_ACT_* (derivative from the output, gm_act.hpp)
__global__ __launch_bounds__(256) void k_leaky_bwd(const float* __restrict__ gy, const float* __restrict__ y,
                                                   long long rows, int cols, int rows_per_block, float slope,
                                                   int act, int fromz, float* __restrict__ g,
                                                   float* __restrict__ part, unsigned* __restrict__ amax) {
    const long long r0 = (long long)blockIdx.x * rows_per_block;
    const long long r1 = min(rows, r0 + rows_per_block);
    float m = 0.f;
    for (int c = threadIdx.x; c < cols; c += blockDim.x) {
        float acc = 0.f;
        for (long long r = r0; r < r1; r++) {
            const long long i = r * cols + c;
            // torch: input > 0 ? g : slope g; fromz: y holds the pre-activation z (gm_act_bwd_z)
            const float v = act < 0 ? (y[i] > 0.f ? gy[i] : slope * gy[i])
                                    : gy[i] * (fromz ? gm_act_dz(y[i], act) : gm_act_dy(y[i], act));
            g[i] = v;
            acc += v;
            m = fmaxf(m, fabsf(v));
        }
        part[(long long)blockIdx.x * cols + c] = acc;
    }
    if (amax) gm_block_amax(amax, m);
}

static int act_bwd(const char* fn, const float* gy, const float* y, int64_t rows, int32_t cols, float slope, int act,
                   float* g, float* part, int32_t rows_per_block, float* g_scale, void* stream, int fromz = 0) {
    if (!gy || !y || !g || !part || rows <= 0 || cols <= 0 || rows_per_block <= 0)
        return gm_fail(GM_ERR_INVALID_ARG, std::string(fn) + ": bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if (g_scale && hipMemsetAsync(g_scale, 0, sizeof(float), st) != hipSuccess)
        return gm_fail(GM_ERR_HIP, std::string(fn) + ": memset");
    const long long nb = (rows + rows_per_block - 1) / rows_per_block;
    hipLaunchKernelGGL(k_leaky_bwd, dim3((unsigned)nb), dim3(256), 0, st, gy, y, (long long)rows, (int)cols,
                       (int)rows_per_block, slope, act, fromz, g, part, reinterpret_cast<unsigned*>(g_scale));
    int rc = launched();
    if (rc == GM_OK && g_scale) rc = gm_absmax_finish(g_scale, stream);
    return rc;
}

extern "C" int gm_leaky_bwd(const float* gy, const float* y, int64_t rows, int32_t cols, float slope, float* g,
                            float* part, int32_t rows_per_block, float* g_scale, void* stream) {
    return act_bwd("gm_leaky_bwd", gy, y, rows, cols, slope, -1, g, part, rows_per_block, g_scale, stream);
}

extern "C" int gm_act_bwd(const float* gy, const float* y, int64_t rows, int32_t cols, int32_t act, float* g,
                          float* part, int32_t rows_per_block, float* g_scale, void* stream) {
    if (act < GM_ACT_NONE || act > GM_ACT_SOFTPLUS)
        return gm_fail(GM_ERR_INVALID_ARG, "gm_act_bwd: unknown act (codes >= GM_ACT_GELU: gm_act_bwd_z)");
    return act_bwd("gm_act_bwd", gy, y, rows, cols, 0.f, act, g, part, rows_per_block, g_scale, stream);
}

extern "C" int gm_act_bwd_z(const float* gy, const float* z, int64_t rows, int32_t cols, int32_t act, float* g,
                            float* part, int32_t rows_per_block, float* g_scale, void* stream) {
    if (act < GM_ACT_NONE || act > GM_ACT_LAST) return gm_fail(GM_ERR_INVALID_ARG, "gm_act_bwd_z: unknown act");
    return act_bwd("gm_act_bwd_z", gy, z, rows, cols, 0.f, act, g, part, rows_per_block, g_scale, stream, 1);
}

// y = act(z) elementwise (the training forward of the activations whose derivative needs z)
__global__ __launch_bounds__(256) void k_act_fwd(const float* __restrict__ z, long long n, int act, float* __restrict__ y) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        y[i] = gm_act(z[i], act);
}

extern "C" int gm_act_fwd(const float* z, int64_t rows, int32_t cols, int32_t act, float* y, void* stream) {
    if (!z || !y || rows <= 0 || cols <= 0 || act < GM_ACT_NONE || act > GM_ACT_LAST)
        return gm_fail(GM_ERR_INVALID_ARG, "gm_act_fwd: bad arguments");
    const long long n = (long long)rows * cols;
    long long nb = (n + 255) / 256;
    if (nb > 65536) nb = 65536;
    hipLaunchKernelGGL(k_act_fwd, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, z, n, (int)act, y);
    return launched();
}

extern "C" int gm_mp_aggregate(const float* h, const int32_t* nbr, int32_t G, int32_t N, int32_t deg, int32_t H,
                               int32_t mode, float* out, void* stream) {
    if (!h || !nbr || !out || G <= 0 || N <= 0 || deg < 0 || deg > MAXDEG || H <= 0 || mode < 0 || mode > 1)
        return gm_fail(GM_ERR_INVALID_ARG, "gm_mp_aggregate: bad arguments (deg <= 8)");
    return launch_agg<false>(h, nbr, G, N, deg, H, mode, out, stream);
}

extern "C" int gm_mp_aggregate_rows(const float* h, int64_t ldh, const int32_t* nbr, int32_t G, int32_t N, int32_t deg,
                                    int32_t H, int32_t mode, float* out, int64_t ldo, void* stream) {
    if (!h || !nbr || !out || G <= 0 || N <= 0 || deg < 0 || deg > MAXDEG || H <= 0 || mode < 0 || mode > 1 ||
        ldh < H || ldo < H)
        return gm_fail(GM_ERR_INVALID_ARG, "gm_mp_aggregate_rows: bad arguments (deg <= 8, ld >= H)");
    return launch_agg<false>(h, nbr, G, N, deg, H, mode, out, stream, ldh, ldo);
}

extern "C" int gm_mp_aggregate_bwd(const float* dout, const int32_t* nbr, int32_t G, int32_t N, int32_t deg,
                                   int32_t H, int32_t mode, float* dh, void* stream) {
    if (!dout || !nbr || !dh || G <= 0 || N <= 0 || deg < 0 || deg > MAXDEG || H <= 0 || mode < 0 || mode > 1)
        return gm_fail(GM_ERR_INVALID_ARG, "gm_mp_aggregate_bwd: bad arguments");
    return launch_agg<true>(dout, nbr, G, N, deg, H, mode, dh, stream);
}

// gm_mp_iterate[_bwd]: K rounds in one LDS-resident launch where the graph fits and the rows are 16-byte lanes,
// the chained per-round launches otherwise (gm_mp_iterate_set_form: -1 per shape, 0 chain, 1 LDS where eligible)
static int g_iterate_form = -1;
extern "C" int gm_mp_iterate_set_form(int32_t form) {
    if (form < -1 || form > 1) return gm_fail(GM_ERR_INVALID_ARG, "gm_mp_iterate_set_form: form -1, 0 or 1");
    g_iterate_form = form;
    return GM_OK;
}

namespace {
constexpr int MP_ITER_MAX_NODES = 65536;      // per graph (header: gm_mp_iterate)
constexpr size_t MP_ITER_LDS_MAX = 160 * 1024;  // LDS of a CU: one block may take all of it
struct IterPlan { bool lds; int P, gpb, threads; size_t bytes; };

inline bool al16(const void* p, long long ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0; }

// LDS form: rows of 16-byte lanes, at most 1024 lanes per row, both images of one graph within a CU's LDS.
// Small graphs are packed until a block's first sweep is full (256 threads); a block whose images leave room
// for no second block on the CU runs 1024 threads instead.
IterPlan iter_plan(int G, int N, int deg, int H, int iters, bool aligned) {
    IterPlan p{false, 0, 1, 256, 0};
    if (!aligned || H % 4 != 0 || H / 4 > 1024 || iters < 1 || g_iterate_form == 0) return p;
    const int HV = H / 4;
    p.P = H % 64 == 0 ? H : H + 4;
    auto bytes = [&](int gpb) {
        return (size_t)gpb * N * (2 * (size_t)p.P * 4 + (size_t)(deg + 1) * 4 + 8);
    };
    if (bytes(1) > MP_ITER_LDS_MAX) return p;
    int gpb = 1;
    while (gpb < 16 && (long long)gpb * N * HV < 256 && bytes(gpb + 1) <= 40 * 1024) gpb++;
    p.gpb = gpb;
    p.bytes = bytes(gpb);
    p.threads = p.bytes > 80 * 1024 ? 1024 : 256;
    if (HV > p.threads) p.threads = 1024;
    p.threads = p.threads / HV * HV;
    // K = 1 has nothing to fuse: the chained form is the copy of h0 into prev plus one aggregate launch (4 images
    // moved against 3). Measured: the LDS form wins 11-12 % in the class of small graphs with several
    // blocks per CU (N = 20, H = 128) and ties where a block fills most of a CU's LDS (N = 100), which stays chained
    p.lds = g_iterate_form == 1 || iters >= 2 || p.bytes <= 40 * 1024;
    return p;
}

template <bool BWD>
int launch_iterate(const IterPlan& p, const float* src, long long lds, const float* add, long long lda,
                   const int32_t* nbr, int G, int N, int deg, int H, int mode, int iters, float* out, long long ldo,
                   float* prev, long long ldp, void* stream) {
    // more than 64 KB of dynamic LDS needs the limit raised; set per call (cheap next to such a launch, and right
    // for every thread and device)
    if (p.bytes > 64 * 1024 &&
        hipFuncSetAttribute((const void*)(k_mp_iterate<BWD>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)MP_ITER_LDS_MAX) != hipSuccess)
        return gm_fail(GM_ERR_HIP, "gm_mp_iterate: raising the LDS limit failed");
    GM_RAN(BWD ? "k_mp_iterate<bwd>" : "k_mp_iterate<fwd>");
    hipLaunchKernelGGL(k_mp_iterate<BWD>, dim3((unsigned)((G + p.gpb - 1) / p.gpb)), dim3(p.threads), p.bytes,
                       (hipStream_t)stream, src, lds, add, lda, nbr, G, N, deg, H, p.P, p.gpb, mode, iters, out, ldo,
                       prev, ldp);
    return launched();
}
}  // namespace

extern "C" int gm_mp_iterate(const float* h0, int64_t ld0, const int32_t* nbr, int32_t G, int32_t N, int32_t deg,
                             int32_t H, int32_t mode, int32_t iters, float* out, int64_t ldo, float* prev,
                             int64_t ldp, void* stream) {
    if (!h0 || !nbr || !out || G <= 0 || N <= 0 || deg < 0 || deg > MAXDEG || H <= 0 || mode < 0 || mode > 1 ||
        ld0 < H || ldo < H || (prev && ldp < H))
        return gm_fail(GM_ERR_INVALID_ARG, "gm_mp_iterate: bad arguments (deg <= 8, ld >= H)");
    if (iters < 0) return gm_fail(GM_ERR_INVALID_ARG, "gm_mp_iterate: iters < 0");
    if (iters >= 1 && !prev) return gm_fail(GM_ERR_INVALID_ARG, "gm_mp_iterate: prev is required for iters >= 1");
    if (N > MP_ITER_MAX_NODES) return gm_fail(GM_ERR_INVALID_ARG, "gm_mp_iterate: n_nodes > 65536");
    if (out == h0 || prev == h0 || out == prev)
        return gm_fail(GM_ERR_INVALID_ARG, "gm_mp_iterate: h0, out and prev must be three buffers");
    const bool aligned = al16(h0, ld0) && al16(out, ldo) && al16(prev, ldp);
    const IterPlan p = iter_plan(G, N, deg, H, iters, aligned);
    if (p.lds)
        return launch_iterate<false>(p, h0, ld0, nullptr, 0, nbr, G, N, deg, H, mode, iters, out, ldo, prev, ldp, stream);
    if (iters == 0) {
        int V = std::min(vec_width(H, ld0, h0), vec_width(H, ldo, out));
        if (prev) V = std::min(V, vec_width(H, ldp, prev));
        const long long rows = (long long)G * N;
        GM_VLAUNCH(k_mp_copy_rows, V, dim3(nblocks(rows * (H / V), 256)), h0, (long long)ld0, rows, H / V, out,
                   (long long)ldo, prev, (long long)ldp);
        return launched();
    }
    // chained launches: h_r lands in out when K - r is even, in prev otherwise (K = 1: prev is a copy of h0)
    if (iters == 1) {
        const int V = std::min(vec_width(H, ld0, h0), vec_width(H, ldp, prev));
        const long long rows = (long long)G * N;
        GM_VLAUNCH(k_mp_copy_rows, V, dim3(nblocks(rows * (H / V), 256)), h0, (long long)ld0, rows, H / V, prev,
                   (long long)ldp, (float*)nullptr, 0ll);
        const int rc = launched();
        if (rc != GM_OK) return rc;
    }
    const float* in = h0;
    long long ldi = ld0;
    for (int r = 1; r <= iters; r++) {
        float* dst = (iters - r) % 2 == 0 ? out : prev;
        const long long ldd = (iters - r) % 2 == 0 ? ldo : ldp;
        const int rc = launch_agg<false>(in, nbr, G, N, deg, H, mode, dst, stream, ldi, ldd);
        if (rc != GM_OK) return rc;
        in = dst;
        ldi = ldd;
    }
    return GM_OK;
}

extern "C" int gm_mp_iterate_bwd(const float* d_out, int64_t ldd, const float* d_prev, int64_t ldq,
                                 const int32_t* nbr, int32_t G, int32_t N, int32_t deg, int32_t H, int32_t mode,
                                 int32_t iters, float* d_h0, int64_t ld, void* stream) {
    if (!d_out || !nbr || !d_h0 || G <= 0 || N <= 0 || deg < 0 || deg > MAXDEG || H <= 0 || mode < 0 || mode > 1 ||
        ldd < H || ld < H || (d_prev && ldq < H))
        return gm_fail(GM_ERR_INVALID_ARG, "gm_mp_iterate_bwd: bad arguments (deg <= 8, ld >= H)");
    if (iters < 0) return gm_fail(GM_ERR_INVALID_ARG, "gm_mp_iterate_bwd: iters < 0");
    if (N > MP_ITER_MAX_NODES) return gm_fail(GM_ERR_INVALID_ARG, "gm_mp_iterate_bwd: n_nodes > 65536");
    if (d_h0 == d_out || d_h0 == d_prev)
        return gm_fail(GM_ERR_INVALID_ARG, "gm_mp_iterate_bwd: d_h0 must not alias an input");
    hipStream_t st = (hipStream_t)stream;
    const long long rows = (long long)G * N;
    if (iters == 0) {
        const int V = std::min(vec_width(H, ldd, d_out), vec_width(H, ld, d_h0));
        GM_VLAUNCH(k_mp_copy_rows, V, dim3(nblocks(rows * (H / V), 256)), d_out, (long long)ldd, rows, H / V, d_h0,
                   (long long)ld, (float*)nullptr, 0ll);
        return launched();
    }
    const bool aligned = al16(d_out, ldd) && al16(d_h0, ld) && al16(d_prev, ldq);
    const IterPlan p = iter_plan(G, N, deg, H, iters, aligned);
    if (p.lds)
        return launch_iterate<true>(p, d_out, ldd, d_prev, ldq, nbr, G, N, deg, H, mode, iters, d_h0, ld, nullptr, 0,
                                    stream);
    // chained launches: one stream-ordered scratch image for the ping-pong of K >= 2
    float* tmp = nullptr;
    if (iters >= 2 && hipMallocAsync((void**)&tmp, (size_t)rows * H * sizeof(float), st) != hipSuccess)
        return gm_fail(GM_ERR_OOM, "gm_mp_iterate_bwd: scratch allocation failed");
    // round r = 1..K writes d_h0 when K - r is even, the scratch otherwise
    const float* in = d_out;
    long long ldi = ldd;
    int rc = GM_OK;
    for (int r = 1; r <= iters && rc == GM_OK; r++) {
        float* dst = (iters - r) % 2 == 0 ? d_h0 : tmp;
        const long long ldt = (iters - r) % 2 == 0 ? (long long)ld : (long long)H;
        rc = launch_agg<true>(in, nbr, G, N, deg, H, mode, dst, stream, ldi, ldt);
        if (rc == GM_OK && r == 1 && d_prev) {
            const int V = std::min(vec_width(H, ldt, dst), vec_width(H, ldq, d_prev));
            GM_VLAUNCH(k_mp_add_rows, V, dim3(nblocks(rows * (H / V), 256)), dst, ldt, d_prev, (long long)ldq, rows,
                       H / V);
            rc = launched();
        }
        in = dst;
        ldi = ldt;
    }
    if (tmp && hipFreeAsync(tmp, st) != hipSuccess && rc == GM_OK) rc = gm_fail(GM_ERR_HIP, "gm_mp_iterate_bwd: free");
    return rc;
}

// readout, one wave per output row (the row's node and neighbour ids read once, as wave-uniform
// loads), 16-byte lanes over the (deg + 1) * H columns; two rows per iteration keep 4 independent
// loads in flight per lane. Requires H % 4 == 0 and 16-byte aligned rows (host-checked).
__global__ __launch_bounds__(256) void k_readout_rows(const float* __restrict__ hf, const float* __restrict__ hp,
                                                      const int32_t* __restrict__ nbr,
                                                      const int32_t* __restrict__ agent_node, long long rows, int N,
                                                      int R, int deg, int H, float* __restrict__ out,
                                                      long long stride, long long ldf, long long ldp) {
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nw = ((long long)gridDim.x * blockDim.x) >> 6;
    const int H4 = H >> 2, W4 = (deg + 1) * H4;
    // U rows per iteration: their node ids first, then every row's loads, then the stores
    constexpr int U = 4, C = 2;  // C float4 per lane and row cover W4 <= 128 (larger W4: the loop below)
    for (long long rb = wave * U; rb < rows; rb += nw * U) {
        long long src[U][C];
        float* dst[U];
        bool okc[U][C];
#pragma unroll
        for (int k = 0; k < U; k++) {
            const long long row = min(rb + k, rows - 1);
            const long long g = row / R;
            const int r = (int)(row - g * R);
            const int v = agent_node ? agent_node[row] : r;
            dst[k] = (rb + k < rows) ? out + row * stride : nullptr;
#pragma unroll
            for (int cc = 0; cc < C; cc++) {
                const int c = lane + 64 * cc;
                const int seg = c / H4, off = (c - seg * H4) * 4;
                okc[k][cc] = c < W4;
                const int m = seg == 0 ? v : (c < W4 ? nbr[(g * N + v) * deg + seg - 1] : -1);
                src[k][cc] = m < 0 ? -1 : (seg == 0 ? (g * N + m) * ldf + off : -(2 + (g * N + m) * ldp + off));
            }
        }
        float4 val[U][C];
#pragma unroll
        for (int k = 0; k < U; k++)
#pragma unroll
            for (int cc = 0; cc < C; cc++) {
                const long long o = src[k][cc];
                val[k][cc] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (okc[k][cc] && o != -1) val[k][cc] = o >= 0 ? *reinterpret_cast<const float4*>(hf + o)
                                                                : *reinterpret_cast<const float4*>(hp + (-o - 2));
            }
#pragma unroll
        for (int k = 0; k < U; k++)
#pragma unroll
            for (int cc = 0; cc < C; cc++)
                if (dst[k] && okc[k][cc]) *reinterpret_cast<float4*>(dst[k] + 4 * (lane + 64 * cc)) = val[k][cc];
        for (int k = 0; k < U && W4 > 64 * C; k++) {  // columns past 64 C float4 (wide readouts)
            const long long row = rb + k;
            if (row >= rows) break;
            const long long g = row / R;
            const int r = (int)(row - g * R);
            const int v = agent_node ? agent_node[row] : r;
            for (int c = lane + 64 * C; c < W4; c += 64) {
                const int seg = c / H4, off = (c - seg * H4) * 4;
                float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                if (seg == 0) {
                    x = *reinterpret_cast<const float4*>(hf + (g * N + v) * ldf + off);
                } else {
                    const int m = nbr[(g * N + v) * deg + seg - 1];
                    if (m >= 0) x = *reinterpret_cast<const float4*>(hp + (g * N + m) * ldp + off);
                }
                *reinterpret_cast<float4*>(out + row * stride + 4 * c) = x;
            }
        }
    }
}

// readout backward, one block per graph: the graph's R output rows ((deg + 1) H floats each) are
// staged in LDS with coalesced 16-byte loads, then thread (node, 4 columns) sums the rows that read
// it in the same (row, segment) order as k_readout_bwd (identical results)
__global__ __launch_bounds__(1024) void k_readout_bwd_lds(const float* __restrict__ dout, long long stride,
                                                          const int32_t* __restrict__ nbr,
                                                          const int32_t* __restrict__ agent_node, int N, int R,
                                                          int deg, int H, float* __restrict__ dhf,
                                                          float* __restrict__ dhp) {
    extern __shared__ float sd[];  // [R][(deg + 1) H]
    __shared__ int su[64];
    __shared__ int snb[64 * MAXDEG];
    const long long g = blockIdx.x;
    const int W = (deg + 1) * H, W4 = W >> 2;
    for (int i = threadIdx.x; i < R; i += blockDim.x) su[i] = agent_node ? agent_node[g * R + i] : i;
    for (int i = threadIdx.x; i < R * W4; i += blockDim.x) {
        const int r = i / W4, c = i - r * W4;
        reinterpret_cast<float4*>(sd)[i] = *reinterpret_cast<const float4*>(dout + (g * R + r) * stride + 4 * c);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < R * deg; i += blockDim.x) {
        const int r = i / deg, k = i - r * deg;
        snb[i] = nbr[(g * N + su[r]) * deg + k];
    }
    __syncthreads();
    const int H4 = H >> 2;
    for (int t = threadIdx.x; t < N * H4; t += blockDim.x) {
        const int v = t / H4, off = (t - v * H4) * 4;
        float4 af = make_float4(0.f, 0.f, 0.f, 0.f), ap = af;
        for (int r = 0; r < R; r++) {
            const float* drow = sd + r * W;
            if (su[r] == v) af = f4add(af, *reinterpret_cast<const float4*>(drow + off));
            for (int k = 0; k < deg; k++)
                if (snb[r * deg + k] == v) ap = f4add(ap, *reinterpret_cast<const float4*>(drow + (k + 1) * H + off));
        }
        const long long node = g * N + v;
        if (dhf) *reinterpret_cast<float4*>(dhf + node * H + off) = af;
        if (dhp) *reinterpret_cast<float4*>(dhp + node * H + off) = ap;
    }
}

// k_readout_bwd_lds over S column chunks per graph (block = (graph, chunk)): 1/S of the LDS per
// block, so S times as many blocks stay resident. The (row, segment) -> node map is inverted once per
// block into per-node row bitmasks (LDS atomic OR: order-free; MW 64-bit words per mask, rows up to
// 64 MW: every node of a 100-node graph without agent map), so a (node, column) thread visits only the
// rows that read its node, in ascending (row, segment) order: the same summation order as
// k_readout_bwd (identical results).
template <int MW>
__global__ __launch_bounds__(256) void k_readout_bwd_cs(const float* __restrict__ dout, long long stride,
                                                        const int32_t* __restrict__ nbr,
                                                        const int32_t* __restrict__ agent_node, int N, int R, int deg,
                                                        int H, int S, float* __restrict__ dhf, float* __restrict__ dhp) {
    extern __shared__ float4 sq[];  // [R][deg + 1][C4]
    __shared__ int su[64 * MW];
    __shared__ unsigned long long smask[128][4][MW];  // node -> rows reading it, per segment (deg <= 3)
    const long long g = blockIdx.x / S;
    const int cs = blockIdx.x - (int)(g * S);
    const int C4 = (H >> 2) / S, SEG = deg + 1;
    for (int i = threadIdx.x; i < R; i += blockDim.x) su[i] = agent_node ? agent_node[g * R + i] : i;
    for (int i = threadIdx.x; i < N * SEG * MW; i += blockDim.x) smask[i / (SEG * MW)][(i / MW) % SEG][i % MW] = 0ull;
    for (int i = threadIdx.x; i < R * SEG * C4; i += blockDim.x) {
        const int r = i / (SEG * C4), rem = i - r * SEG * C4, sg = rem / C4, c = rem - sg * C4;
        sq[i] = *reinterpret_cast<const float4*>(dout + (g * R + r) * stride + sg * H + (cs * C4 + c) * 4);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < R * SEG; e += blockDim.x) {
        const int r = e / SEG, sg = e - r * SEG;
        const int v = sg == 0 ? su[r] : nbr[(g * N + su[r]) * deg + sg - 1];
        if (v >= 0 && v < N) atomicOr(&smask[v][sg][r >> 6], 1ull << (r & 63));
    }
    __syncthreads();
    for (int t = threadIdx.x; t < N * C4; t += blockDim.x) {
        const int v = t / C4, c = t - v * C4;
        float4 af = make_float4(0.f, 0.f, 0.f, 0.f), ap = af;
#pragma unroll
        for (int w = 0; w < MW; w++)
            for (unsigned long long m = smask[v][0][w]; m; m &= m - 1)
                af = f4add(af, sq[(64 * w + __ffsll(m) - 1) * SEG * C4 + c]);
#pragma unroll
        for (int w = 0; w < MW; w++) {
            unsigned long long mk[3], any = 0ull;
            for (int k = 0; k < deg; k++) any |= (mk[k] = smask[v][k + 1][w]);
            for (; any; any &= any - 1) {
                const int rb = __ffsll(any) - 1, r = 64 * w + rb;
                for (int k = 0; k < deg; k++)
                    if ((mk[k] >> rb) & 1ull) ap = f4add(ap, sq[(r * SEG + k + 1) * C4 + c]);
            }
        }
        const long long o = (g * N + v) * H + (cs * C4 + c) * 4;
        if (dhf) *reinterpret_cast<float4*>(dhf + o) = af;
        if (dhp) *reinterpret_cast<float4*>(dhp + o) = ap;
    }
}

// Readout backward without an agent map (every node reads itself out: config 5's all-nodes readout,
// src/sl.py:132-168): row v of dout is [dh_final(v) | dh_prev(nbr(v, 0)) | ... ], so dhf(u) is row u's
// segment 0 and dhp(u) = sum over the neighbours v of u, ascending, of row v's segment 1 + (slot of u in v's
// ascending list) (symmetric adjacency: u is in v's list once). A gather per (node, 16-B chunk) instead of the
// per-graph LDS staging of k_readout_bwd_cs; the same ascending-row order, so the same fp32 sums
template <typename I>
__global__ __launch_bounds__(256) void k_readout_bwd_nodes(const float* __restrict__ dout, long long stride,
                                                           const int32_t* __restrict__ nbr, long long nodes, int N,
                                                           int deg, int H, float* __restrict__ dhf,
                                                           float* __restrict__ dhp) {
    // I: the index type of the (node, chunk) decomposition, 32-bit when nodes * H / 4 fits (no 64-bit division)
    const I C4 = (I)(H >> 2);
    const I t = (I)blockIdx.x * (I)blockDim.x + (I)threadIdx.x;
    if ((long long)t >= nodes * C4) return;
    const I u = t / C4;
    const int c = (int)(t - u * C4);
    const I g0 = (u / (I)N) * (I)N;
    const int ul = (int)(u - g0);
    const long long U = (long long)u, G0 = (long long)g0;
    if (dhf) *reinterpret_cast<float4*>(dhf + U * H + 4 * c) = *reinterpret_cast<const float4*>(dout + U * stride + 4 * c);
    if (!dhp) return;
    // all neighbour ids, then all their lists, then all gradient loads in flight together; summed in ascending k
    // as before (the same fp32 sums)
    int v[MAXDEG], slot[MAXDEG];
#pragma unroll
    for (int k = 0; k < MAXDEG; k++) v[k] = k < deg ? nbr[U * deg + k] : -1;
#pragma unroll
    for (int k = 0; k < MAXDEG; k++) {
        slot[k] = -1;
        if (v[k] >= 0 && v[k] < N)
            for (int j = 0; j < deg; j++)
                if (nbr[(G0 + v[k]) * deg + j] == ul) slot[k] = j;
    }
    float4 x[MAXDEG];
#pragma unroll
    for (int k = 0; k < MAXDEG; k++)
        x[k] = slot[k] >= 0 ? *reinterpret_cast<const float4*>(dout + (G0 + v[k]) * stride + (1 + slot[k]) * H + 4 * c)
                            : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 ap = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < MAXDEG; k++)
        if (slot[k] >= 0) ap = f4add(ap, x[k]);
    *reinterpret_cast<float4*>(dhp + U * H + 4 * c) = ap;
}

extern "C" int gm_netmon_readout_ld(const float* hf, int64_t ldf, const float* hp, int64_t ldp, const int32_t* nbr,
                                    const int32_t* agent_node, int32_t G, int32_t N, int32_t R, int32_t deg, int32_t H,
                                    float* out, int64_t stride, void* stream) {
    if (!hf || !hp || !nbr || !out || G <= 0 || N <= 0 || R <= 0 || deg < 0 || H <= 0 ||
        stride < (int64_t)(deg + 1) * H || ldf < H || ldp < H)
        return gm_fail(GM_ERR_INVALID_ARG, "gm_netmon_readout: bad arguments");
    if (!agent_node && R != N) return gm_fail(GM_ERR_INVALID_ARG, "gm_netmon_readout: R must equal N without agent map");
    int V = vec_width(H, stride, out);
    int v2 = vec_width(H, ldf, hf), v3 = vec_width(H, ldp, hp);
    V = V < v2 ? V : v2;
    V = V < v3 ? V : v3;
    if (V == 4) {
        const long long rows = (long long)G * R;
        const long long blocks = std::min<long long>((rows + 3) / 4, 65536);
        GM_RAN("k_readout_rows");
        hipLaunchKernelGGL(k_readout_rows, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, hf, hp, nbr,
                           agent_node, rows, N, R, deg, H, out, (long long)stride, (long long)ldf, (long long)ldp);
        return launched();
    }
    long long total = (long long)G * R * (deg + 1) * (H / V);
    GM_VLAUNCH(k_readout, V, dim3(nblocks(total, 256)), hf, hp, nbr, agent_node, G, N, R, deg, H, out,
               (long long)stride, (long long)ldf, (long long)ldp);
    return launched();
}

extern "C" int gm_netmon_readout(const float* hf, const float* hp, const int32_t* nbr, const int32_t* agent_node,
                                 int32_t G, int32_t N, int32_t R, int32_t deg, int32_t H, float* out, int64_t stride,
                                 void* stream) {
    return gm_netmon_readout_ld(hf, H, hp, H, nbr, agent_node, G, N, R, deg, H, out, stride, stream);
}

// Same gather, one block per graph: the graph's agent nodes and their neighbour lists are
// staged in LDS once (the per-thread version re-read them from L1/L2 for every node and column
// chunk), then every (node, column chunk) thread sums its contributions in the same (agent,
// segment) order as k_readout_bwd, so the results are identical.
template <int V>
__global__ __launch_bounds__(1024) void k_readout_bwd_g(const float* __restrict__ dout, long long stride,
                                                        const int32_t* __restrict__ nbr,
                                                        const int32_t* __restrict__ agent_node, int N, int R, int deg,
                                                        int H, float* __restrict__ dhf, float* __restrict__ dhp) {
    __shared__ int su[64];
    __shared__ int snb[64 * MAXDEG];
    const long long g = blockIdx.x;
    for (int i = threadIdx.x; i < R; i += blockDim.x) su[i] = agent_node ? agent_node[g * R + i] : i;
    __syncthreads();
    for (int i = threadIdx.x; i < R * deg; i += blockDim.x) {
        const int r = i / deg, k = i - r * deg;
        snb[i] = nbr[(g * N + su[r]) * deg + k];
    }
    __syncthreads();
    const int HV = H / V;
    if ((int)threadIdx.x >= N * HV) return;
    const int v = threadIdx.x / HV, off = (threadIdx.x % HV) * V;
    Vec<V> af = zerov<V>(), ap = zerov<V>();
    for (int r = 0; r < R; r++) {
        const float* drow = dout + (g * R + r) * stride;
        if (su[r] == v) {
            Vec<V> x = ldv<V>(drow + off);
#pragma unroll
            for (int i = 0; i < V; i++) af.v[i] += x.v[i];
        }
        for (int k = 0; k < deg; k++) {
            if (snb[r * deg + k] == v) {
                Vec<V> x = ldv<V>(drow + (size_t)(k + 1) * H + off);
#pragma unroll
                for (int i = 0; i < V; i++) ap.v[i] += x.v[i];
            }
        }
    }
    const long long node = g * N + v;
    if (dhf) stv<V>(dhf + node * H + off, af);
    if (dhp) stv<V>(dhp + node * H + off, ap);
}

// sym: the caller vouches for a symmetric neighbour table without repeated entries (gm_netmon_readout_bwd_sym);
// only then may the no-map call take k_readout_bwd_nodes, which is silently wrong on any other table
static int readout_bwd(const float* dout, int64_t stride, const int32_t* nbr, const int32_t* agent_node, int32_t G,
                       int32_t N, int32_t R, int32_t deg, int32_t H, float* dhf, float* dhp, bool sym, void* stream) {
    if (!dout || !nbr || G <= 0 || N <= 0 || R <= 0 || deg < 0 || H <= 0)
        return gm_fail(GM_ERR_INVALID_ARG, "gm_netmon_readout_bwd: bad arguments");
    int V = vec_width(H, stride, dout);
    if (dhf) { int v = vec_width(H, H, dhf); V = V < v ? V : v; }
    if (dhp) { int v = vec_width(H, H, dhp); V = V < v ? V : v; }
    if (!agent_node && R != N)
        return gm_fail(GM_ERR_INVALID_ARG, "gm_netmon_readout_bwd: R must equal N without agent map");
    if (sym && !agent_node && V == 4 && deg <= MAXDEG) {  // symmetric table, every node read out: a gather per node
        const long long total = (long long)G * N * (H / 4);
        if (total + 256 < (1ll << 31)) {
            GM_RAN("k_readout_bwd_nodes<unsigned>");
            hipLaunchKernelGGL(k_readout_bwd_nodes<unsigned>, dim3(nblocks(total, 256)), dim3(256), 0,
                               (hipStream_t)stream, dout, (long long)stride, nbr, (long long)G * N, N, deg, H, dhf, dhp);
        } else {
            GM_RAN("k_readout_bwd_nodes<long long>");
            hipLaunchKernelGGL(k_readout_bwd_nodes<long long>, dim3(nblocks(total, 256)), dim3(256), 0,
                               (hipStream_t)stream, dout, (long long)stride, nbr, (long long)G * N, N, deg, H, dhf, dhp);
        }
        return launched();
    }
    const size_t lds = (size_t)R * (deg + 1) * H * 4;
    // column chunks per graph: 4, or 8 when a quarter of the graph's rows exceeds 48 KB of LDS
    const int S = (lds / 4 <= 48 * 1024 || (H / 4) % 8) ? 4 : 8;
    if (V == 4 && R <= 128 && N <= 128 && deg <= 3 && (H / 4) % S == 0 && lds / S <= 48 * 1024) {
        const int threads = std::min(256, (N * (H / (4 * S)) + 63) / 64 * 64);
        if (R <= 64) {
            GM_RAN(S == 4 ? "k_readout_bwd_cs<1>/S=4" : "k_readout_bwd_cs<1>/S=8");
            hipLaunchKernelGGL(k_readout_bwd_cs<1>, dim3((unsigned)((long long)G * S)), dim3(threads), lds / S,
                               (hipStream_t)stream, dout, (long long)stride, nbr, agent_node, N, R, deg, H, S, dhf, dhp);
        } else {  // up to 128 rows per graph (e.g. every node of a 100-node graph, no agent map)
            GM_RAN(S == 4 ? "k_readout_bwd_cs<2>/S=4" : "k_readout_bwd_cs<2>/S=8");
            hipLaunchKernelGGL(k_readout_bwd_cs<2>, dim3((unsigned)((long long)G * S)), dim3(threads), lds / S,
                               (hipStream_t)stream, dout, (long long)stride, nbr, agent_node, N, R, deg, H, S, dhf, dhp);
        }
        return launched();
    }
    if (V == 4 && R <= 64 && deg <= MAXDEG && lds <= 48 * 1024) {
        const int threads = std::min(1024, (N * (H / 4) + 63) / 64 * 64);
        GM_RAN("k_readout_bwd_lds");
        hipLaunchKernelGGL(k_readout_bwd_lds, dim3(G), dim3(threads), lds, (hipStream_t)stream, dout, (long long)stride,
                           nbr, agent_node, N, R, deg, H, dhf, dhp);
        return launched();
    }
    if (R <= 64 && deg <= MAXDEG && N * (H / V) <= 1024) {
        const int threads = (N * (H / V) + 63) / 64 * 64;
        hipStream_t st = (hipStream_t)stream;
        GM_RAN(V == 4 ? "k_readout_bwd_g<4>" : V == 2 ? "k_readout_bwd_g<2>" : "k_readout_bwd_g<1>");
        if (V == 4)
            hipLaunchKernelGGL(k_readout_bwd_g<4>, dim3(G), dim3(threads), 0, st, dout, (long long)stride, nbr,
                               agent_node, N, R, deg, H, dhf, dhp);
        else if (V == 2)
            hipLaunchKernelGGL(k_readout_bwd_g<2>, dim3(G), dim3(threads), 0, st, dout, (long long)stride, nbr,
                               agent_node, N, R, deg, H, dhf, dhp);
        else
            hipLaunchKernelGGL(k_readout_bwd_g<1>, dim3(G), dim3(threads), 0, st, dout, (long long)stride, nbr,
                               agent_node, N, R, deg, H, dhf, dhp);
        return launched();
    }
    long long total = (long long)G * N * (H / V);
    GM_VLAUNCH(k_readout_bwd, V, dim3(nblocks(total, 256)), dout, (long long)stride, nbr, agent_node, G, N, R, deg, H,
               dhf, dhp);
    return launched();
}

extern "C" int gm_netmon_readout_bwd(const float* dout, int64_t stride, const int32_t* nbr, const int32_t* agent_node,
                                     int32_t G, int32_t N, int32_t R, int32_t deg, int32_t H, float* dhf, float* dhp,
                                     void* stream) {
    return readout_bwd(dout, stride, nbr, agent_node, G, N, R, deg, H, dhf, dhp, false, stream);
}

extern "C" int gm_netmon_readout_bwd_sym(const float* dout, int64_t stride, const int32_t* nbr, int32_t G, int32_t N,
                                         int32_t deg, int32_t H, float* dhf, float* dhp, void* stream) {
    return readout_bwd(dout, stride, nbr, nullptr, G, N, N, deg, H, dhf, dhp, true, stream);
}

// Global-mean readout (--netmon-global, src/model.py:458-469, 624-627): the mean of h over a graph's nodes,
// broadcast to the graph's output rows. A block owns gpb whole graphs; a thread owns one V-float column chunk of
// one graph (lanes run along H, so every row access is contiguous), sums the N node rows in ascending order in
// fp32 (the value does not depend on the launch shape) and stores the mean into the graph's R rows. No atomics.
template <int V>
__global__ __launch_bounds__(256) void k_global_rows(const float* __restrict__ state, long long lds, int G, int N,
                                                     int HV, int R, int gpb, float* __restrict__ out,
                                                     long long ldo) {
    const float inv = 1.0f / (float)N;
    for (int i = threadIdx.x; i < gpb * HV; i += blockDim.x) {
        const int gl = i / HV, c = (i - gl * HV) * V;
        const long long g = (long long)blockIdx.x * gpb + gl;
        if (g >= G) break;  // gl ascends with i
        const float* s = state + g * N * lds + c;
        Vec<V> acc = zerov<V>();
#pragma unroll 4
        for (int n = 0; n < N; n++) {
            const Vec<V> x = ldv<V>(s + n * lds);
#pragma unroll
            for (int k = 0; k < V; k++) acc.v[k] += x.v[k];
        }
#pragma unroll
        for (int k = 0; k < V; k++) acc.v[k] *= inv;
        float* o = out + g * R * ldo + c;
        for (int r = 0; r < R; r++) stv<V>(o + r * ldo, acc);
    }
}

// Its transpose, accumulated: dh[node n of graph g] += (1/N) * (sum over the graph's rows r, ascending, of d_rows).
// The same ownership (one thread per graph and column chunk), so plain loads and stores suffice.
template <int V>
__global__ __launch_bounds__(256) void k_global_bwd(const float* __restrict__ d, long long ldd, int G, int N, int HV,
                                                    int R, int gpb, float* __restrict__ dh, long long ldh) {
    const float inv = 1.0f / (float)N;
    for (int i = threadIdx.x; i < gpb * HV; i += blockDim.x) {
        const int gl = i / HV, c = (i - gl * HV) * V;
        const long long g = (long long)blockIdx.x * gpb + gl;
        if (g >= G) break;
        const float* s = d + g * R * ldd + c;
        Vec<V> acc = zerov<V>();
#pragma unroll 4
        for (int r = 0; r < R; r++) {
            const Vec<V> x = ldv<V>(s + r * ldd);
#pragma unroll
            for (int k = 0; k < V; k++) acc.v[k] += x.v[k];
        }
#pragma unroll
        for (int k = 0; k < V; k++) acc.v[k] *= inv;
        float* o = dh + g * N * ldh + c;
        for (int n = 0; n < N; n++) {
            Vec<V> x = ldv<V>(o + n * ldh);
#pragma unroll
            for (int k = 0; k < V; k++) x.v[k] += acc.v[k];
            stv<V>(o + n * ldh, x);
        }
    }
}

static bool global_args_ok(const void* a, int64_t lda, int32_t G, int32_t N, int32_t H, int32_t R, const void* b,
                           int64_t ldb) {
    return a && b && G > 0 && N > 0 && N <= 128 && R > 0 && H > 0 && H % 32 == 0 && H <= 1024 && lda >= H &&
           ldb >= H && (reinterpret_cast<uintptr_t>(a) & 3) == 0 && (reinterpret_cast<uintptr_t>(b) & 3) == 0;
}

// graphs per block: 256 threads' worth of column chunks, one graph when a graph has that many
static int global_gpb(int HV) { return HV >= 256 ? 1 : 256 / HV; }

extern "C" int gm_netmon_global_rows(const float* state, int64_t ld_state, int32_t G, int32_t N, int32_t H,
                                     int32_t R, float* out, int64_t ld_out, void* stream) {
    if (!global_args_ok(state, ld_state, G, N, H, R, out, ld_out))
        return gm_fail(GM_ERR_INVALID_ARG,
                       "gm_netmon_global_rows: bad arguments (hidden % 32 == 0, hidden <= 1024, n_nodes <= 128, ld >= hidden)");
    const int v0 = vec_width(H, ld_state, state), v1 = vec_width(H, ld_out, out);
    const int V = v0 < v1 ? v0 : v1;  // scalar dword stores when the output base or stride is not 8 / 16-byte aligned
    const int HV = H / V, gpb = global_gpb(HV);
    GM_VLAUNCH(k_global_rows, V, dim3(nblocks(G, gpb)), state, (long long)ld_state, (int)G, (int)N, HV, (int)R, gpb, out,
               (long long)ld_out);
    return launched();
}

extern "C" int gm_netmon_global_bwd(const float* d_rows, int64_t ld_d, int32_t G, int32_t N, int32_t H, int32_t R,
                                    float* dh, int64_t ld_dh, void* stream) {
    if (!global_args_ok(d_rows, ld_d, G, N, H, R, dh, ld_dh))
        return gm_fail(GM_ERR_INVALID_ARG,
                       "gm_netmon_global_bwd: bad arguments (hidden % 32 == 0, hidden <= 1024, n_nodes <= 128, ld >= hidden)");
    const int v0 = vec_width(H, ld_d, d_rows), v1 = vec_width(H, ld_dh, dh);
    const int V = v0 < v1 ? v0 : v1;
    const int HV = H / V, gpb = global_gpb(HV);
    GM_VLAUNCH(k_global_bwd, V, dim3(nblocks(G, gpb)), d_rows, (long long)ld_d, (int)G, (int)N, HV, (int)R, gpb, dh,
               (long long)ld_dh);
    return launched();
}

extern "C" int gm_lstm_pointwise(const float* gates, const float* c, int32_t m, int32_t H, float* h1, float* c1,
                                 float* act, void* stream) {
    if (!gates || !c || !h1 || !c1 || m <= 0 || H <= 0) return gm_fail(GM_ERR_INVALID_ARG, "gm_lstm_pointwise: bad args");
    long long total = (long long)m * H;
    GM_RAN("k_lstm_pw");
    hipLaunchKernelGGL(k_lstm_pw, dim3(nblocks(total, 256)), dim3(256), 0, (hipStream_t)stream, gates, c, m, H, h1, c1,
                       act);
    return launched();
}

extern "C" int gm_lstm_pointwise_bwd(const float* dh1, const float* dc1, const float* act, const float* c,
                                     const float* c1, int32_t m, int32_t H, float* dgates, float* dc,
                                     float* dgates_scale, void* stream) {
    if (!act || !c || !c1 || !dgates || !dc || m <= 0 || H <= 0)
        return gm_fail(GM_ERR_INVALID_ARG, "gm_lstm_pointwise_bwd: bad args");
    hipStream_t st = (hipStream_t)stream;
    if (dgates_scale && hipMemsetAsync(dgates_scale, 0, sizeof(float), st) != hipSuccess)
        return gm_fail(GM_ERR_HIP, "gm_lstm_pointwise_bwd: memset");
    long long total = (long long)m * H;
    // grid-stride over at most 4096 blocks: one published max per block
    const long long nb = std::min<long long>(nblocks(total, 256), 4096);
    GM_RAN("k_lstm_pw_bwd");
    hipLaunchKernelGGL(k_lstm_pw_bwd, dim3((unsigned)nb), dim3(256), 0, st, dh1, dc1, act, c, c1, m, H, dgates, dc,
                       reinterpret_cast<unsigned*>(dgates_scale));
    int rc = launched();
    if (rc == GM_OK && dgates_scale) rc = gm_absmax_finish(dgates_scale, stream);
    return rc;
}

// ---------------------------------------------------------------------------
// Sequence-batched training backward (graph-marl_amd/train_seq.py)
// ---------------------------------------------------------------------------
namespace {

// max over the block through LDS (any block size <= 1024), published once per block
__device__ void block_max_publish(float m, unsigned* slot) {
    __shared__ float red[1024];
    red[threadIdx.x] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < (int)blockDim.x; i++) m = fmaxf(m, red[i]);
        gm_amax_publish(slot, m);
    }
}

// LSTM cell backward with its gradient sources summed on the fly (gm_lstm_cell_bwd). Thread
// (rl, u) of a block of RL x H threads owns unit u of the rows r0 + rl, r0 + rl + RL, ... of the
// block's rows_per_block rows: loads and stores are unit-contiguous; the per-block bias sums are
// the RL row lanes combined in LDS in a fixed order.
__global__ __launch_bounds__(1024) void k_lstm_cell_bwd(gm_lstm_bwd_args a, unsigned* sc_slot, unsigned* max_slot) {
    __shared__ float red[4][1024];
    const int H = a.hidden, RL = blockDim.x / H;
    const int u = threadIdx.x % H, rl = threadIdx.x / H;
    const long long r0 = (long long)blockIdx.x * a.rows_per_block;
    const long long r1 = min((long long)a.m, r0 + a.rows_per_block);
    float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f, mx = 0.f;
    for (long long r = r0 + rl; r < r1; r += RL) {
        const float* ar = a.act + r * a.ld_act + u;
        const float gi = ar[0], gf = ar[H], gg = ar[2 * H], go = ar[3 * H];
        const float c = a.c_in[r * a.ld_cin + u];
        const float tc = tanhf(a.c_out[r * a.ld_cout + u]);
        float dh = 0.f;
        if (a.dh0) dh += a.dh0[r * a.ld_dh0 + u];
        if (a.dh1) dh += a.dh1[r * a.ld_dh1 + u];
        if (a.dm) {  // transpose of the (I + A) aggregate: members of row r's node, ascending id
            const int N = a.n_nodes;
            const long long g = r / N;
            const int n = (int)(r - g * N);
            int mem[MAXDEG + 1];
            const int cnt = members(a.nbr + r * a.deg, a.deg, n, mem);
            for (int q = 0; q < cnt; q++) {
                float v = a.dm[(g * N + mem[q]) * a.ld_dm + u];
                if (a.mean) {
                    const int32_t* nbm = a.nbr + (g * N + mem[q]) * a.deg;
                    int cm = 1;
                    for (int k = 0; k < a.deg; k++) cm += nbm[k] >= 0;
                    v = v * (1.0f / (float)cm);
                }
                dh += v;
            }
        }
        float dcn = a.dc ? a.dc[r * a.ld_dc + u] : 0.f;
        const bool ext = !a.ext_mask || !a.ext_mask[r / a.rows_per_sample];
        if (ext) {
            if (a.dh_ext) dh += a.dh_ext[r * a.ld_ext + u];
            if (a.dc_ext) dcn += a.dc_ext[r * a.ld_dcext + u];
        }
        const float dct = dcn + dh * go * (1.f - tc * tc);
        const float d0 = dct * gg * gi * (1.f - gi), d1 = dct * c * gf * (1.f - gf);
        const float d2 = dct * gi * (1.f - gg * gg), d3 = dh * tc * go * (1.f - go);
        float* dg = a.dgates + r * a.ld_dg + u;
        dg[0] = d0;
        dg[H] = d1;
        dg[2 * H] = d2;
        dg[3 * H] = d3;
        if (a.dc_out) a.dc_out[r * a.ld_dco + u] = dct * gf;
        p0 += d0;
        p1 += d1;
        p2 += d2;
        p3 += d3;
        mx = fmaxf(mx, fmaxf(fmaxf(fabsf(d0), fabsf(d1)), fmaxf(fabsf(d2), fabsf(d3))));
    }
    if (a.bias_part) {
        red[0][threadIdx.x] = p0;
        red[1][threadIdx.x] = p1;
        red[2][threadIdx.x] = p2;
        red[3][threadIdx.x] = p3;
        __syncthreads();
        if (rl == 0) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                float s = red[k][u];
                for (int l = 1; l < RL; l++) s += red[k][l * H + u];
                a.bias_part[(long long)blockIdx.x * 4 * H + k * H + u] = s;
            }
        }
        __syncthreads();
    }
    if (sc_slot || max_slot) {
        __shared__ float mred[1024];
        mred[threadIdx.x] = mx;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int i = 1; i < (int)blockDim.x; i++) mx = fmaxf(mx, mred[i]);
            if (sc_slot) gm_amax_publish(sc_slot, mx);
            if (max_slot) gm_amax_publish(max_slot, mx);
        }
    }
}

// k_lstm_cell_bwd with 4 consecutive units per thread (16-byte loads and stores; every ld and base
// 16-byte aligned, H % 4 == 0): thread (rl, u4) of RL x H/4 threads; per element the same arithmetic
// in the same order as k_lstm_cell_bwd. Bias partials: the RL row lanes combined in LDS in a fixed
// order; max |dgates| per wave, then over the block's waves.
__global__ __launch_bounds__(256) void k_lstm_cell_bwd4(gm_lstm_bwd_args a, unsigned* sc_slot, unsigned* max_slot) {
    __shared__ float4 red[4][256];
    __shared__ float wmx[4];
    const int H = a.hidden, H4 = H >> 2, RL = blockDim.x / H4;
    const int u = (threadIdx.x % H4) * 4, rl = threadIdx.x / H4;
    const long long r0 = (long long)blockIdx.x * a.rows_per_block;
    const long long r1 = min((long long)a.m, r0 + a.rows_per_block);
    auto ld4 = [](const float* p) { return *reinterpret_cast<const float4*>(p); };
    auto add4 = [](float4& x, float4 y) {
        x.x += y.x;
        x.y += y.y;
        x.z += y.z;
        x.w += y.w;
    };
    float4 p[4];
#pragma unroll
    for (int k = 0; k < 4; k++) p[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    float mx = 0.f;
    for (long long r = r0 + rl; r < r1; r += RL) {
        const float* ar = a.act + r * a.ld_act + u;
        const float4 gi4 = ld4(ar), gf4 = ld4(ar + H), gg4 = ld4(ar + 2 * H), go4 = ld4(ar + 3 * H);
        const float4 c4 = ld4(a.c_in + r * a.ld_cin + u), co4 = ld4(a.c_out + r * a.ld_cout + u);
        float4 dh4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.dh0) add4(dh4, ld4(a.dh0 + r * a.ld_dh0 + u));
        if (a.dh1) add4(dh4, ld4(a.dh1 + r * a.ld_dh1 + u));
        if (a.dm) {
            const int N = a.n_nodes;
            const long long g = r / N;
            const int n = (int)(r - g * N);
            int mem[MAXDEG + 1];
            const int cnt = members(a.nbr + r * a.deg, a.deg, n, mem);
            for (int q = 0; q < cnt; q++) {
                float4 v = ld4(a.dm + (g * N + mem[q]) * a.ld_dm + u);
                if (a.mean) {
                    const int32_t* nbm = a.nbr + (g * N + mem[q]) * a.deg;
                    int cm = 1;
                    for (int k = 0; k < a.deg; k++) cm += nbm[k] >= 0;
                    const float f = 1.0f / (float)cm;
                    v = make_float4(v.x * f, v.y * f, v.z * f, v.w * f);
                }
                add4(dh4, v);
            }
        }
        float4 dc4 = a.dc ? ld4(a.dc + r * a.ld_dc + u) : make_float4(0.f, 0.f, 0.f, 0.f);
        const bool ext = !a.ext_mask || !a.ext_mask[r / a.rows_per_sample];
        if (ext) {
            if (a.dh_ext) add4(dh4, ld4(a.dh_ext + r * a.ld_ext + u));
            if (a.dc_ext) add4(dc4, ld4(a.dc_ext + r * a.ld_dcext + u));
        }
        const float* gi = &gi4.x;
        const float* gf = &gf4.x;
        const float* gg = &gg4.x;
        const float* go = &go4.x;
        const float* c = &c4.x;
        const float* co = &co4.x;
        const float* dh = &dh4.x;
        const float* dcn = &dc4.x;
        float4 o0, o1, o2, o3, oc;
        float* d0 = &o0.x;
        float* d1 = &o1.x;
        float* d2 = &o2.x;
        float* d3 = &o3.x;
        float* dco = &oc.x;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const float tc = tanhf(co[e]);
            const float dct = dcn[e] + dh[e] * go[e] * (1.f - tc * tc);
            d0[e] = dct * gg[e] * gi[e] * (1.f - gi[e]);
            d1[e] = dct * c[e] * gf[e] * (1.f - gf[e]);
            d2[e] = dct * gi[e] * (1.f - gg[e] * gg[e]);
            d3[e] = dh[e] * tc * go[e] * (1.f - go[e]);
            dco[e] = dct * gf[e];
            mx = fmaxf(mx, fmaxf(fmaxf(fabsf(d0[e]), fabsf(d1[e])), fmaxf(fabsf(d2[e]), fabsf(d3[e]))));
        }
        float* dg = a.dgates + r * a.ld_dg + u;
        *reinterpret_cast<float4*>(dg) = o0;
        *reinterpret_cast<float4*>(dg + H) = o1;
        *reinterpret_cast<float4*>(dg + 2 * H) = o2;
        *reinterpret_cast<float4*>(dg + 3 * H) = o3;
        if (a.dc_out) *reinterpret_cast<float4*>(a.dc_out + r * a.ld_dco + u) = oc;
        add4(p[0], o0);
        add4(p[1], o1);
        add4(p[2], o2);
        add4(p[3], o3);
    }
    if (a.bias_part) {
#pragma unroll
        for (int k = 0; k < 4; k++) red[k][threadIdx.x] = p[k];
        __syncthreads();
        if (rl == 0) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                float4 s = red[k][threadIdx.x];
                for (int l = 1; l < RL; l++) add4(s, red[k][l * H4 + threadIdx.x]);
                *reinterpret_cast<float4*>(a.bias_part + (long long)blockIdx.x * 4 * H + k * H + u) = s;
            }
        }
    }
    if (sc_slot || max_slot) {
        mx = gm_wave_max(mx);
        if ((threadIdx.x & 63) == 0) wmx[threadIdx.x >> 6] = mx;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < (int)(blockDim.x >> 6); w++) mx = fmaxf(mx, wmx[w]);
            if (sc_slot) gm_amax_publish(sc_slot, mx);
            if (max_slot) gm_amax_publish(max_slot, mx);
        }
    }
}

// Q head + leaky hidden layer backward (gm_qhead_bwd): thread c owns column c of the block's rows
__global__ __launch_bounds__(1024) void k_qhead_bwd(const float* __restrict__ dq, long long ldq, int nq,
                                                   const float* __restrict__ wq, long long ldwq,
                                                   const float* __restrict__ y, long long ldy, long long rows, int cols,
                                                   int act, float* __restrict__ g, long long ldg,
                                                   float* __restrict__ part_b, float* __restrict__ part_wq,
                                                   float* __restrict__ part_bq, int rpb, unsigned* __restrict__ amax) {
    const int c = threadIdx.x;
    const bool ok = c < cols;
    float w[4] = {0.f, 0.f, 0.f, 0.f};
    for (int q = 0; q < nq; q++) w[q] = ok ? wq[q * ldwq + c] : 0.f;
    const long long r0 = (long long)blockIdx.x * rpb, r1 = min(rows, r0 + rpb);
    float pb = 0.f, mx = 0.f, pw[4] = {0.f, 0.f, 0.f, 0.f}, pq[4] = {0.f, 0.f, 0.f, 0.f};
    // U rows per iteration with their loads issued together (independent HBM round trips in flight)
    constexpr int U = 8;
    for (long long rb = r0; rb < r1; rb += U) {
        float d[U][4], yv[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const long long r = min(rb + u, r1 - 1);
#pragma unroll
            for (int q = 0; q < 4; q++) d[u][q] = q < nq ? dq[r * ldq + q] : 0.f;
            yv[u] = ok ? y[r * ldy + c] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (rb + u >= r1) break;
            const long long r = rb + u;
#pragma unroll
            for (int q = 0; q < 4; q++) pq[q] += d[u][q];
            if (ok) {
                float gv = 0.f;
#pragma unroll
                for (int q = 0; q < 4; q++) gv = fmaf(d[u][q], w[q], gv);
                if (act) gv *= gm_act_dy(yv[u], act);
                g[r * ldg + c] = gv;
                pb += gv;
                mx = fmaxf(mx, fabsf(gv));
#pragma unroll
                for (int q = 0; q < 4; q++) pw[q] = fmaf(d[u][q], yv[u], pw[q]);
            }
        }
    }
    if (ok) {
        part_b[(long long)blockIdx.x * cols + c] = pb;
        for (int q = 0; q < nq; q++) part_wq[((long long)blockIdx.x * nq + q) * cols + c] = pw[q];
    }
    if (c == 0)
        for (int q = 0; q < nq; q++) part_bq[(long long)blockIdx.x * nq + q] = pq[q];
    if (amax) block_max_publish(mx, amax);
}

// k_qhead_bwd with 4 columns per thread (16-byte loads / stores; cols % 4 == 0, 16-byte bases and
// strides): RL row lanes x cols/4 threads, U rows per lane in flight; per element the arithmetic of
// k_qhead_bwd; the row lanes' partial sums combined in LDS in a fixed order.
__global__ __launch_bounds__(256) void k_qhead_bwd4(const float* __restrict__ dq, long long ldq, int nq,
                                                   const float* __restrict__ wq, long long ldwq,
                                                   const float* __restrict__ y, long long ldy, long long rows, int cols,
                                                   int act, float* __restrict__ g, long long ldg,
                                                   float* __restrict__ part_b, float* __restrict__ part_wq,
                                                   float* __restrict__ part_bq, int rpb, unsigned* __restrict__ amax) {
    __shared__ float4 red[5][256];
    __shared__ float rq[4][256];
    __shared__ float wmx[4];
    const int C4 = cols >> 2, RL = blockDim.x / C4;
    const int c4 = threadIdx.x % C4, rl = threadIdx.x / C4, c = 4 * c4;
    float4 w[4];
#pragma unroll
    for (int q = 0; q < 4; q++)
        w[q] = q < nq ? *reinterpret_cast<const float4*>(wq + q * ldwq + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    const long long r0 = (long long)blockIdx.x * rpb, r1 = min(rows, r0 + rpb);
    float4 pb = make_float4(0.f, 0.f, 0.f, 0.f), pw[4];
    float pq[4] = {0.f, 0.f, 0.f, 0.f}, mx = 0.f;
#pragma unroll
    for (int q = 0; q < 4; q++) pw[q] = pb;
    constexpr int U = 4;
    for (long long rb = r0 + rl; rb < r1; rb += (long long)U * RL) {
        float d[U][4];
        float4 yv[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const long long r = min(rb + (long long)u * RL, r1 - 1);
#pragma unroll
            for (int q = 0; q < 4; q++) d[u][q] = q < nq ? dq[r * ldq + q] : 0.f;
            yv[u] = *reinterpret_cast<const float4*>(y + r * ldy + c);
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const long long r = rb + (long long)u * RL;
            if (r >= r1) break;
            if (c4 == 0)
#pragma unroll
                for (int q = 0; q < 4; q++) pq[q] += d[u][q];
            const float* ye = &yv[u].x;
            float4 gv4;
            float* gv = &gv4.x;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                float v = 0.f;
#pragma unroll
                for (int q = 0; q < 4; q++) v = fmaf(d[u][q], (&w[q].x)[e], v);
                if (act) v *= gm_act_dy(ye[e], act);
                gv[e] = v;
                mx = fmaxf(mx, fabsf(v));
            }
            *reinterpret_cast<float4*>(g + r * ldg + c) = gv4;
            pb.x += gv4.x;
            pb.y += gv4.y;
            pb.z += gv4.z;
            pb.w += gv4.w;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                pw[q].x = fmaf(d[u][q], ye[0], pw[q].x);
                pw[q].y = fmaf(d[u][q], ye[1], pw[q].y);
                pw[q].z = fmaf(d[u][q], ye[2], pw[q].z);
                pw[q].w = fmaf(d[u][q], ye[3], pw[q].w);
            }
        }
    }
    red[0][threadIdx.x] = pb;
#pragma unroll
    for (int q = 0; q < 4; q++) red[1 + q][threadIdx.x] = pw[q];
    if (c4 == 0)
#pragma unroll
        for (int q = 0; q < 4; q++) rq[q][rl] = pq[q];
    __syncthreads();
    if (rl == 0) {
        for (int k = 0; k <= nq; k++) {
            float4 sm = red[k][c4];
            for (int l = 1; l < RL; l++) {
                const float4 o = red[k][l * C4 + c4];
                sm.x += o.x;
                sm.y += o.y;
                sm.z += o.z;
                sm.w += o.w;
            }
            float* dst = k == 0 ? part_b + (long long)blockIdx.x * cols : part_wq + ((long long)blockIdx.x * nq + k - 1) * cols;
            *reinterpret_cast<float4*>(dst + c) = sm;
        }
        if (c4 == 0)
            for (int q = 0; q < nq; q++) {
                float sm = rq[q][0];
                for (int l = 1; l < RL; l++) sm += rq[q][l];
                part_bq[(long long)blockIdx.x * nq + q] = sm;
            }
    }
    if (amax) {
        mx = gm_wave_max(mx);
        if ((threadIdx.x & 63) == 0) wmx[threadIdx.x >> 6] = mx;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int k = 1; k < (int)(blockDim.x >> 6); k++) mx = fmaxf(mx, wmx[k]);
            gm_amax_publish(amax, mx);
        }
    }
}

}  // namespace

extern "C" int gm_lstm_cell_bwd(const gm_lstm_bwd_args* a, void* stream) {
    if (!a || !a->act || !a->c_in || !a->c_out || !a->dgates || a->m <= 0 || a->hidden <= 0 || a->hidden > 1024 ||
        (a->hidden > 256 && a->hidden % 64) || (a->dm && (!a->nbr || a->n_nodes <= 0 || a->deg < 0 || a->deg > MAXDEG)) ||
        (a->ext_mask && a->rows_per_sample <= 0) || (a->bias_part && a->rows_per_block <= 0))
        return gm_fail(GM_ERR_INVALID_ARG, "gm_lstm_cell_bwd: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const int H = a->hidden;
    const int RL = H >= 256 ? 1 : 256 / H;
    const int threads = H * RL;
    gm_lstm_bwd_args b = *a;
    if (b.rows_per_block <= 0) b.rows_per_block = 64;
    if (b.dg_scale && hipMemsetAsync(b.dg_scale, 0, sizeof(float), st) != hipSuccess)
        return gm_fail(GM_ERR_HIP, "gm_lstm_cell_bwd: memset");
    const long long nb = (b.m + b.rows_per_block - 1) / b.rows_per_block;
    auto a16 = [](const void* p, long long ld) { return !p || ((reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0); };
    const bool vec = H % 4 == 0 && H / 4 <= 256 && ((256 / (H / 4)) * (H / 4)) % 64 == 0 &&
                     a16(b.act, b.ld_act) && a16(b.c_in, b.ld_cin) && a16(b.c_out, b.ld_cout) &&
                     a16(b.dh0, b.ld_dh0) && a16(b.dh1, b.ld_dh1) && a16(b.dm, b.ld_dm) && a16(b.dh_ext, b.ld_ext) &&
                     a16(b.dc_ext, b.ld_dcext) && a16(b.dc, b.ld_dc) && a16(b.dgates, b.ld_dg) &&
                     a16(b.dc_out, b.ld_dco) && a16(b.bias_part, 4);
    if (vec) {
        const int rl4 = 256 / (H / 4);
        GM_RAN("k_lstm_cell_bwd4");
        hipLaunchKernelGGL(k_lstm_cell_bwd4, dim3((unsigned)nb), dim3(rl4 * (H / 4)), 0, st, b,
                           reinterpret_cast<unsigned*>(b.dg_scale), reinterpret_cast<unsigned*>(b.dg_max));
    } else {
        GM_RAN("k_lstm_cell_bwd");
        hipLaunchKernelGGL(k_lstm_cell_bwd, dim3((unsigned)nb), dim3(threads), 0, st, b,
                           reinterpret_cast<unsigned*>(b.dg_scale), reinterpret_cast<unsigned*>(b.dg_max));
    }
    int rc = launched();
    if (rc == GM_OK && b.dg_scale) rc = gm_absmax_finish(b.dg_scale, stream);
    return rc;
}

extern "C" int gm_qhead_bwd(const float* dq, int64_t ldq, int32_t nq, const float* wq, int64_t ldwq, const float* y,
                            int64_t ldy, int64_t rows, int32_t cols, int32_t act, float* g, int64_t ldg, float* part_b,
                            float* part_wq, float* part_bq, int32_t rows_per_block, float* g_scale, void* stream) {
    if (!dq || !wq || !y || !g || !part_b || !part_wq || !part_bq || nq <= 0 || nq > 4 || rows <= 0 || cols <= 0 ||
        cols > 1024 || ldq < nq || ldwq < cols || ldy < cols || ldg < cols || rows_per_block <= 0)
        return gm_fail(GM_ERR_INVALID_ARG, "gm_qhead_bwd: bad arguments (nq <= 4, cols <= 1024)");
    hipStream_t st = (hipStream_t)stream;
    if (g_scale && hipMemsetAsync(g_scale, 0, sizeof(float), st) != hipSuccess)
        return gm_fail(GM_ERR_HIP, "gm_qhead_bwd: memset");
    const long long nb = (rows + rows_per_block - 1) / rows_per_block;
    auto a16 = [](const void* p, long long ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0; };
    if (cols % 4 == 0 && cols <= 1024 && ((256 / (cols / 4)) * (cols / 4)) % 64 == 0 && a16(wq, ldwq) &&
        a16(y, ldy) && a16(g, ldg) && a16(part_b, cols) && a16(part_wq, cols)) {
        const int rl = 256 / (cols / 4);
        GM_RAN("k_qhead_bwd4");
        hipLaunchKernelGGL(k_qhead_bwd4, dim3((unsigned)nb), dim3(rl * (cols / 4)), 0, st, dq, (long long)ldq, nq, wq,
                           (long long)ldwq, y, (long long)ldy, (long long)rows, cols, act, g, (long long)ldg, part_b,
                           part_wq, part_bq, rows_per_block, reinterpret_cast<unsigned*>(g_scale));
        int rc = launched();
        if (rc == GM_OK && g_scale) rc = gm_absmax_finish(g_scale, stream);
        return rc;
    }
    const int threads = (cols + 63) / 64 * 64;
    GM_RAN("k_qhead_bwd");
    hipLaunchKernelGGL(k_qhead_bwd, dim3((unsigned)nb), dim3(threads), 0, st, dq, (long long)ldq, nq, wq,
                       (long long)ldwq, y, (long long)ldy, (long long)rows, cols, act, g, (long long)ldg, part_b,
                       part_wq, part_bq, rows_per_block, reinterpret_cast<unsigned*>(g_scale));
    int rc = launched();
    if (rc == GM_OK && g_scale) rc = gm_absmax_finish(g_scale, stream);
    return rc;
}

extern "C" int gm_routing_node_encoder(const float* x, int64_t ldx, const int32_t* nbr, int32_t G, int32_t N,
                                       const float* wt, const float* b, int32_t n, int32_t act, float* y, int64_t ldy,
                                       void* stream) {
    return gm_routing_node_encoder_bits(x, ldx, nbr, G, N, wt, b, n, act, y, ldy, nullptr, 0, stream);
}

extern "C" int gm_routing_node_encoder_bits(const float* x, int64_t ldx, const int32_t* nbr, int32_t G, int32_t N,
                                            const float* wt, const float* b, int32_t n, int32_t act, float* y,
                                            int64_t ldy, uint32_t* sbits, int64_t ldsb, void* stream) {
    if (!x || !nbr || !wt || !y || G <= 0 || N < 4 || n <= 0 || (n % 64) || act < GM_ACT_NONE || act > GM_ACT_LAST ||
        ldx < 4 * N + 8 || ldy < n || (ldy % 2) || (reinterpret_cast<uintptr_t>(wt) & 15) ||
        (reinterpret_cast<uintptr_t>(y) & 7) || (sbits && ldsb < n / 32))
        return gm_fail(GM_ERR_INVALID_ARG,
                       "gm_routing_node_encoder: bad arguments (n % 64 == 0, 16-byte W^T, 8-byte y, even ldy)");
    const int K = 4 * N + 8;
    // columns per lane: 2 while the block's W^T slice (K x 128 floats) fits 64 KB (N <= 30), else 1 (2 above
    // N = 30 with a slice of up to 160 KB at one block per CU measured within noise, round 4)
    const int cpl = (n % 128 == 0 && (size_t)K * 128 * 4 <= 65536) ? 2 : 1;
    const size_t lds = (size_t)K * 64 * cpl * 4;
    if (lds > 160 * 1024) return gm_fail(GM_ERR_UNSUPPORTED, "gm_routing_node_encoder: 4N+8 too large for the LDS slice");
    const long long M = (long long)G * N;
    // 8 waves per block share the staged W^T slice; rows per block grow with the graph size (the slice is
    // staged once for them). Round 3, interleaved rollout A/B, per-launch times at 4096 envs: N = 20 512
    // rows 54.9 vs 63.8 us (256 rows, 4 waves), N = 30 1024 rows 88.9 vs 111.7 us, N = 40 157.5 vs 170.5
    // us, N = 50 222 vs 240 us
    const int rows = (K <= 88 ? 256 : (K <= 128 ? 512 : 1024)) * (K <= 128 ? 2 : 1);
    dim3 grid((unsigned)((M + rows - 1) / rows), (unsigned)(n / (64 * cpl)));
#define GM_RENC(C, A)                                                                                               \
    do {                                                                                                            \
        GM_RAN(lds > 65536 ? "k_routing_enc<" #C "," #A ">/lds>64K" : "k_routing_enc<" #C "," #A ">");              \
        if (lds > 65536)                                                                                            \
            (void)hipFuncSetAttribute((const void*)(k_routing_enc<C, A, 512>),                                      \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                        \
        hipLaunchKernelGGL((k_routing_enc<C, A, 512>), grid, dim3(512), lds, (hipStream_t)stream, x, (long long)ldx, \
                           nbr, G, N, wt, b, n, act, y, (long long)ldy, rows, reinterpret_cast<unsigned*>(sbits),    \
                           (long long)ldsb);                                                                        \
    } while (0)
    if (cpl == 2) {
        if (act == GM_ACT_LEAKY_RELU) GM_RENC(2, 1);
        else if (act == GM_ACT_NONE) GM_RENC(2, 0);
        else GM_RENC(2, -1);
    } else {
        if (act == GM_ACT_LEAKY_RELU) GM_RENC(1, 1);
        else if (act == GM_ACT_NONE) GM_RENC(1, 0);
        else GM_RENC(1, -1);
    }
#undef GM_RENC
    return launched();
}

// ---------------------------------------------------------------------------
// LayerNorm-LSTM cell after its two gate GEMMs (reference src/layernormlstm.py:24-42):
//   g  = LN_in(x W_ih^T) + LN_hid(h W_hh^T) + b_ih      (LN over the 4H gate pre-activations)
//   c' = LN_cell(sigma(f) c + sigma(i) tanh(g_c)),  h' = sigma(o) tanh(c')   (LN over H)
// One wave per row, the row's 8H raw products (gi | gh, columns in the original gate order)
// held in registers: lane l owns units u = l + 64 q (q < UPL) of all four gates, so every load
// and store is a 64-wide coalesced run and the three LayerNorm statistics are two-pass wave
// reductions over registers (mean, then the sum of squared deviations, like torch's fp32
// LayerNorm, eps 1e-5). HBM-bound: 8H floats in, c in, h' and c' out per row.
// ---------------------------------------------------------------------------
namespace {
__device__ __forceinline__ float wsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// precise expf / tanhf (not the GEMM epilogues' 1e-6 hardware approximations): the cell LayerNorm
// divides by the spread of c, which would amplify gate errors; the kernel is HBM-bound anyway
__device__ __forceinline__ float sig_f(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float tanh_f(float x) { return tanhf(x); }

struct LnLstmP {
    const float *gi_w, *gi_b, *gh_w, *gh_b, *bias, *lc_w, *lc_b;
};

template <int UPL>
__global__ __launch_bounds__(256) void k_lnlstm_pw(const float* __restrict__ Gi, long long ldgi,
                                                   const float* __restrict__ Gh, long long ldgh,
                                                   const float* __restrict__ c_in, long long ldc, LnLstmP p, int M,
                                                   int H, float eps, float* __restrict__ y, long long ldy,
                                                   float* __restrict__ y2, long long ldy2, float* __restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;  // wave-uniform
    const float* gi = Gi + row * ldgi;
    const float* gh = Gh + row * ldgh;
    float a[UPL][4], b[UPL][4];
    float si = 0.f, sh = 0.f;
#pragma unroll
    for (int q = 0; q < UPL; q++) {
        const int u = lane + 64 * q;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool ok = u < H;
            a[q][k] = ok ? gi[k * H + u] : 0.f;
            b[q][k] = ok ? gh[k * H + u] : 0.f;
            si += a[q][k];
            sh += b[q][k];
        }
    }
    const float inv4h = 1.0f / (float)(4 * H);
    const float mi = wsum(si) * inv4h, mh = wsum(sh) * inv4h;
    float vi = 0.f, vh = 0.f;
#pragma unroll
    for (int q = 0; q < UPL; q++)
        if (lane + 64 * q < H)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float di = a[q][k] - mi, dh = b[q][k] - mh;
                vi += di * di;
                vh += dh * dh;
            }
    const float ri = 1.0f / sqrtf(wsum(vi) * inv4h + eps), rh = 1.0f / sqrtf(wsum(vh) * inv4h + eps);
    float cp[UPL], og[UPL], sc = 0.f;
#pragma unroll
    for (int q = 0; q < UPL; q++) {
        const int u = lane + 64 * q;
        cp[q] = og[q] = 0.f;
        if (u >= H) continue;
        float g[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int col = k * H + u;
            g[k] = ((a[q][k] - mi) * ri * p.gi_w[col] + p.gi_b[col]) + ((b[q][k] - mh) * rh * p.gh_w[col] + p.gh_b[col]) +
                   p.bias[col];
        }
        cp[q] = sig_f(g[1]) * c_in[row * ldc + u] + sig_f(g[0]) * tanh_f(g[2]);
        og[q] = sig_f(g[3]);
        sc += cp[q];
    }
    const float invh = 1.0f / (float)H;
    const float mc = wsum(sc) * invh;
    float vc = 0.f;
#pragma unroll
    for (int q = 0; q < UPL; q++)
        if (lane + 64 * q < H) {
            const float d = cp[q] - mc;
            vc += d * d;
        }
    const float rc = 1.0f / sqrtf(wsum(vc) * invh + eps);
#pragma unroll
    for (int q = 0; q < UPL; q++) {
        const int u = lane + 64 * q;
        if (u >= H) continue;
        const float cn = (cp[q] - mc) * rc * p.lc_w[u] + p.lc_b[u];
        y[row * ldy + u] = og[q] * tanh_f(cn);
        y2[row * ldy2 + u] = cn;
    }
    if (stats && lane < 6) {  // the row's LayerNorm statistics for the backward pass
        const float v = lane == 0 ? mi : lane == 1 ? ri : lane == 2 ? mh : lane == 3 ? rh : lane == 4 ? mc : rc;
        stats[row * 8 + lane] = v;
    }
}

// Backward of k_lnlstm_pw (src/layernormlstm.py:24-42 differentiated by hand). One wave per row, the
// same unit ownership as the forward; the forward quantities are recomputed from the raw gate GEMM
// outputs, c and the saved statistics (no activation tensor in HBM). Per row:
//   dcy = dc1 + dh1 o (1 - tanh^2 cy), do = dh1 tanh cy
//   LN_cell^T: dn = dcy w_c, du = r_c (dn - mean dn - n_c mean(dn n_c))
//   di = du g, dg = du i, df = du c, dc = du f; gate pre-activations dG through sigma' / tanh'
//   LN_in^T / LN_hid^T: dni = dG w_i, d gi = r_i (dni - mean dni - n_i mean(dni n_i)) (same for h)
// Parameter gradients are accumulated per wave in registers and written as one partial row per wave:
// part[wave][14H] = [d w_i (4H) | d w_h (4H) | d bias (4H; also d b_i and d b_h) | d w_c (H) | d b_c (H)].

// the per-wave parameter-gradient accumulators of the LayerNorm-LSTM backward kernels
template <int UPL>
struct LnLstmAcc {
    float wi[UPL][4], wh[UPL][4], b[UPL][4], wc[UPL], bc[UPL];
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int q = 0; q < UPL; q++) {
            wc[q] = bc[q] = 0.f;
#pragma unroll
            for (int k = 0; k < 4; k++) wi[q][k] = wh[q][k] = b[q][k] = 0.f;
        }
    }
    __device__ __forceinline__ void store(float* pr, int H, int lane) const {
#pragma unroll
        for (int q = 0; q < UPL; q++) {
            const int u = lane + 64 * q;
            if (u >= H) continue;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                pr[k * H + u] = wi[q][k];
                pr[4 * H + k * H + u] = wh[q][k];
                pr[8 * H + k * H + u] = b[q][k];
            }
            pr[12 * H + u] = wc[q];
            pr[13 * H + u] = bc[q];
        }
    }
};

// One row of the LayerNorm-LSTM backward, in ONE operation order for both kernels that run it (k_lnlstm_bwd and
// k_lnlstm_cell_bwd give the same bits on the same row gradients): gh1 / gc1 = the row's total gradient of h' and
// c' for this lane's units (zero beyond H), dgi / dgh the row's output rows, dco (nullable) the row's d c; the
// parameter gradients go into acc, max |d gi| / |d gh| into mxi / mxh when AMAX.
template <int UPL, bool AMAX>
__device__ __forceinline__ void lnlstm_row_bwd(const float* __restrict__ gi, const float* __restrict__ gh,
                                               const float* __restrict__ cin, const LnLstmP& p,
                                               const float* __restrict__ st, int H, int lane, const float (&gh1)[UPL],
                                               const float (&gc1)[UPL], float* __restrict__ dgi,
                                               float* __restrict__ dgh, float* __restrict__ dco, LnLstmAcc<UPL>& acc,
                                               float& mxi, float& mxh) {
    // every product and sum rounded on its own, so the result does not depend on what the surrounding kernel
    // lets the compiler contract into an fma
#pragma clang fp contract(off)
    const float inv4h = 1.0f / (float)(4 * H), invh = 1.0f / (float)H;
    const float mi = st[0], ri = st[1], mh = st[2], rh = st[3], mc = st[4], rc = st[5];
    float ni[UPL][4], nh[UPL][4], act[UPL][4], cx[UPL], nc[UPL], dcy[UPL], dO[UPL];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int q = 0; q < UPL; q++) {
        const int u = lane + 64 * q;
        cx[q] = nc[q] = dcy[q] = dO[q] = 0.f;
#pragma unroll
        for (int k = 0; k < 4; k++) ni[q][k] = nh[q][k] = act[q][k] = 0.f;
        if (u >= H) continue;
        float g[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int col = k * H + u;
            ni[q][k] = (gi[col] - mi) * ri;
            nh[q][k] = (gh[col] - mh) * rh;
            g[k] = (ni[q][k] * p.gi_w[col] + p.gi_b[col]) + (nh[q][k] * p.gh_w[col] + p.gh_b[col]) + p.bias[col];
        }
        act[q][0] = sig_f(g[0]);
        act[q][1] = sig_f(g[1]);
        act[q][2] = tanh_f(g[2]);
        act[q][3] = sig_f(g[3]);
        cx[q] = cin[u];
        const float cp = act[q][1] * cx[q] + act[q][0] * act[q][2];
        // one unit: the normalised value is 0 whatever c is (LayerNorm of a single element). Computed, it is the
        // rounding of the recomputed cp against the saved mean times rc = 1 / sqrt(eps)
        nc[q] = H == 1 ? 0.f : (cp - mc) * rc;
        const float cy = nc[q] * p.lc_w[u] + p.lc_b[u];
        const float th = tanh_f(cy);
        dcy[q] = gc1[q] + gh1[q] * act[q][3] * (1.f - th * th);
        dO[q] = gh1[q] * th;
        acc.wc[q] += dcy[q] * nc[q];
        acc.bc[q] += dcy[q];
        const float dn = dcy[q] * p.lc_w[u];
        s1 += dn;
        s2 += dn * nc[q];
    }
    const float m1 = wsum(s1) * invh, m2 = wsum(s2) * invh;
    float dG[UPL][4];
    float ti1 = 0.f, ti2 = 0.f, th1 = 0.f, th2 = 0.f;
#pragma unroll
    for (int q = 0; q < UPL; q++) {
        const int u = lane + 64 * q;
#pragma unroll
        for (int k = 0; k < 4; k++) dG[q][k] = 0.f;
        if (u >= H) continue;
        const float du = rc * (dcy[q] * p.lc_w[u] - m1 - nc[q] * m2);
        const float i = act[q][0], f = act[q][1], gg = act[q][2], o = act[q][3];
        if (dco) dco[u] = du * f;
        dG[q][0] = du * gg * i * (1.f - i);
        dG[q][1] = du * cx[q] * f * (1.f - f);
        dG[q][2] = du * i * (1.f - gg * gg);
        dG[q][3] = dO[q] * o * (1.f - o);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int col = k * H + u;
            acc.b[q][k] += dG[q][k];
            acc.wi[q][k] += dG[q][k] * ni[q][k];
            acc.wh[q][k] += dG[q][k] * nh[q][k];
            const float a = dG[q][k] * p.gi_w[col], b = dG[q][k] * p.gh_w[col];
            ti1 += a;
            ti2 += a * ni[q][k];
            th1 += b;
            th2 += b * nh[q][k];
        }
    }
    const float mi1 = wsum(ti1) * inv4h, mi2 = wsum(ti2) * inv4h;
    const float mh1 = wsum(th1) * inv4h, mh2 = wsum(th2) * inv4h;
#pragma unroll
    for (int q = 0; q < UPL; q++) {
        const int u = lane + 64 * q;
        if (u >= H) continue;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int col = k * H + u;
            const float oi = ri * (dG[q][k] * p.gi_w[col] - mi1 - ni[q][k] * mi2);
            const float oh = rh * (dG[q][k] * p.gh_w[col] - mh1 - nh[q][k] * mh2);
            dgi[col] = oi;
            dgh[col] = oh;
            if (AMAX) {
                mxi = fmaxf(mxi, fabsf(oi));
                mxh = fmaxf(mxh, fabsf(oh));
            }
        }
    }
}

template <int UPL>
__global__ __launch_bounds__(256) void k_lnlstm_bwd(const float* __restrict__ Gi, long long ldgi,
                                                    const float* __restrict__ Gh, long long ldgh,
                                                    const float* __restrict__ c_in, long long ldc, LnLstmP p,
                                                    const float* __restrict__ stats, const float* __restrict__ dh1,
                                                    long long lddh, const float* __restrict__ dc1, long long lddc,
                                                    int M, int H, int rpw, float* __restrict__ dgi, long long lddgi,
                                                    float* __restrict__ dgh, long long lddgh, float* __restrict__ dc,
                                                    long long lddco, float* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long r0 = wave * rpw;
    if (r0 >= M) return;  // wave-uniform
    const long long r1 = r0 + rpw < M ? r0 + rpw : M;
    LnLstmAcc<UPL> acc;
    acc.zero();
    float mxi = 0.f, mxh = 0.f;
    for (long long row = r0; row < r1; row++) {
        float gh1[UPL], gc1[UPL];
#pragma unroll
        for (int q = 0; q < UPL; q++) {
            const int u = lane + 64 * q;
            const bool ok = u < H;
            gh1[q] = ok && dh1 ? dh1[row * lddh + u] : 0.f;
            gc1[q] = ok && dc1 ? dc1[row * lddc + u] : 0.f;
        }
        lnlstm_row_bwd<UPL, false>(Gi + row * ldgi, Gh + row * ldgh, c_in + row * ldc, p, stats + row * 8, H, lane,
                                   gh1, gc1, dgi + row * lddgi, dgh + row * lddgh, dc + row * lddco, acc, mxi, mxh);
    }
    acc.store(part + wave * 14LL * H, H, lane);
}

// LayerNorm-LSTM cell backward of the sequence-batched training path (gm_lnlstm_cell_bwd): k_lnlstm_bwd's wave
// and unit ownership and its row math (lnlstm_row_bwd), with the row's gradient of h' and c' summed on the fly
// from every source of the cell as k_lstm_cell_bwd sums them (dh0, dh1, the transposed (I + A) aggregate of dm
// in ascending member order, dh_ext / dc_ext unless the row's sample is masked, dc); each lane gathers its own
// units of at most deg + 1 dm rows in 64-wide runs. max |d gi| and max |d gh| are published once per wave.
template <int UPL>
__global__ __launch_bounds__(256) void k_lnlstm_cell_bwd(gm_lnlstm_cell_bwd_args a, LnLstmP p, unsigned* sci,
                                                         unsigned* sch) {
    const int lane = threadIdx.x & 63;
    const int H = a.hidden, rpw = a.rows_per_wave;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long r0 = wave * rpw;
    if (r0 >= a.m) return;  // wave-uniform
    const long long r1 = r0 + rpw < a.m ? r0 + rpw : a.m;
    LnLstmAcc<UPL> acc;
    acc.zero();
    float mxi = 0.f, mxh = 0.f;
    for (long long row = r0; row < r1; row++) {
        float gh1[UPL], gc1[UPL];
#pragma unroll
        for (int q = 0; q < UPL; q++) gh1[q] = gc1[q] = 0.f;
        int mem[MAXDEG + 1];
        float ms[MAXDEG + 1];
        int cnt = 0;
        long long g0 = 0;  // first row of the row's graph
        if (a.dm) {        // transpose of the (I + A) aggregate: members of the row's node, ascending id
            const int N = a.n_nodes;
            const long long g = row / N;
            g0 = g * N;
            cnt = members(a.nbr + row * a.deg, a.deg, (int)(row - g0), mem);
            for (int e = 0; e < cnt; e++) {
                ms[e] = 1.0f;
                if (a.mean) {
                    const int32_t* nbm = a.nbr + (g0 + mem[e]) * a.deg;
                    int cm = 1;
                    for (int k = 0; k < a.deg; k++) cm += nbm[k] >= 0;
                    ms[e] = 1.0f / (float)cm;
                }
            }
        }
        const bool ext = !a.ext_mask || !a.ext_mask[row / a.rows_per_sample];
#pragma unroll
        for (int q = 0; q < UPL; q++) {
            const int u = lane + 64 * q;
            if (u >= H) continue;
            float dh = 0.f, dcn = 0.f;
            if (a.dh0) dh += a.dh0[row * a.ld_dh0 + u];
            if (a.dh1) dh += a.dh1[row * a.ld_dh1 + u];
            for (int e = 0; e < cnt; e++) {
                float v = a.dm[(g0 + mem[e]) * a.ld_dm + u];
                if (a.mean) v = v * ms[e];
                dh += v;
            }
            if (a.dc) dcn += a.dc[row * a.ld_dc + u];
            if (ext) {
                if (a.dh_ext) dh += a.dh_ext[row * a.ld_ext + u];
                if (a.dc_ext) dcn += a.dc_ext[row * a.ld_dcext + u];
            }
            gh1[q] = dh;
            gc1[q] = dcn;
        }
        lnlstm_row_bwd<UPL, true>(a.gi + row * a.ld_gi, a.gh + row * a.ld_gh, a.c_in + row * a.ld_cin, p,
                                  a.stats + row * 8, H, lane, gh1, gc1, a.dgi + row * a.ld_dgi,
                                  a.dgh + row * a.ld_dgh, a.dc_out ? a.dc_out + row * a.ld_dco : nullptr, acc, mxi,
                                  mxh);
    }
    if (a.part) acc.store(a.part + wave * 14LL * H, H, lane);
    if (sci || a.dgi_max || sch || a.dgh_max) {
        mxi = gm_wave_max(mxi);
        mxh = gm_wave_max(mxh);
        if (lane == 0) {
            if (sci) gm_amax_publish(sci, mxi);
            if (a.dgi_max) gm_amax_publish(reinterpret_cast<unsigned*>(a.dgi_max), mxi);
            if (sch) gm_amax_publish(sch, mxh);
            if (a.dgh_max) gm_amax_publish(reinterpret_cast<unsigned*>(a.dgh_max), mxh);
        }
    }
}

// h' of a GRU cell from its pre-activations a_r, a_z, a_nx, a_nh and the state h, in ONE operation order for
// every kernel that computes it (gm_gru_cell_fwd gives gm_gru_pointwise's bits): the tanh argument is one fma,
// the blend two products and a sum, whatever the surrounding code would let the compiler contract or pack.
__device__ __forceinline__ float gru_gate(float ar, float az, float anx, float anh, float h, float& r, float& z,
                                          float& n) {
#pragma clang fp contract(off)
    r = sig_f(ar);
    z = sig_f(az);
    n = tanh_f(fmaf(r, anh, anx));
    const float t0 = (1.f - z) * n, t1 = z * h;
    return t0 + t1;
}

// GRU cell gate math (torch.nn.GRUCell, gate order r, z, n): gi = x W_ih^T + b_ih, gh = h W_hh^T + b_hh
// ([m][3H] each, strided), r = sigma(gi_r + gh_r), z = sigma(gi_z + gh_z), n = tanh(gi_n + r gh_n),
// h' = (1 - z) n + z h. One thread per (row, unit).
__global__ __launch_bounds__(256) void k_gru_pw(const float* __restrict__ gi, long long ldgi,
                                                const float* __restrict__ gh, long long ldgh,
                                                const float* __restrict__ h, long long ldh, int M, int H,
                                                float* __restrict__ y, long long ldy) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)M * H) return;
    const long long row = t / H;
    const int u = (int)(t - row * H);
    const float* a = gi + row * ldgi;
    const float* b = gh + row * ldgh;
    float r, z, n;
    y[row * ldy + u] =
        gru_gate(a[u] + b[u], a[H + u] + b[H + u], a[2 * H + u], b[2 * H + u], h[row * ldh + u], r, z, n);
}

// Backward of k_gru_pw: dn = dh' (1 - z), dz = dh' (h - n), dh = dh' z; dn_pre = dn (1 - n^2);
// d gi = [dr_pre, dz_pre, dn_pre], d gh = [dr_pre, dz_pre, dn_pre r], dr_pre = dn_pre gh_n r (1 - r),
// dz_pre = dz z (1 - z).
__global__ __launch_bounds__(256) void k_gru_bwd(const float* __restrict__ gi, long long ldgi,
                                                 const float* __restrict__ gh, long long ldgh,
                                                 const float* __restrict__ h, long long ldh,
                                                 const float* __restrict__ dy, long long lddy, int M, int H,
                                                 float* __restrict__ dgi, long long lddgi, float* __restrict__ dgh,
                                                 long long lddgh, float* __restrict__ dh, long long lddh) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)M * H) return;
    const long long row = t / H;
    const int u = (int)(t - row * H);
    const float* a = gi + row * ldgi;
    const float* b = gh + row * ldgh;
    const float r = sig_f(a[u] + b[u]), z = sig_f(a[H + u] + b[H + u]);
    const float ghn = b[2 * H + u];
    const float n = tanh_f(a[2 * H + u] + r * ghn);
    const float g = dy[row * lddy + u], hv = h[row * ldh + u];
    const float dnp = g * (1.f - z) * (1.f - n * n);
    const float drp = dnp * ghn * r * (1.f - r);
    const float dzp = g * (hv - n) * z * (1.f - z);
    dgi[row * lddgi + u] = drp;
    dgi[row * lddgi + H + u] = dzp;
    dgi[row * lddgi + 2 * H + u] = dnp;
    dgh[row * lddgh + u] = drp;
    dgh[row * lddgh + H + u] = dzp;
    dgh[row * lddgh + 2 * H + u] = dnp * r;
    dh[row * lddh + u] = g * z;
}

// GRU cell of the sequence-batched training path (gm_gru_cell_fwd): P = [a_r | a_z | a_nx | a_nh] is the one
// [x | h] GEMM's output on the four-tile weight (fused.pack_gru's blocks in natural order, biases included);
// the same arithmetic as k_gru_pw per (row, unit), V consecutive units per thread; P becomes G = [r | z | n |
// a_nh], what k_gru_cell_bwd reads.
template <int V>
__global__ __launch_bounds__(256) void k_gru_cell_fwd(float* __restrict__ P, long long ldp,
                                                      const float* __restrict__ h, long long ldh, int M, int H,
                                                      float* __restrict__ y, long long ldy) {
    const int HV = H / V;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)M * HV) return;
    const long long row = t / HV;
    const int u = (int)(t - row * HV) * V;
    float* a = P + row * ldp + u;
    const Vec<V> ar = ldv<V>(a), az = ldv<V>(a + H), anx = ldv<V>(a + 2 * H), anh = ldv<V>(a + 3 * H);
    const Vec<V> hv = ldv<V>(h + row * ldh + u);
    Vec<V> r4, z4, n4, o4;
#pragma unroll
    for (int e = 0; e < V; e++) {
        float r, z, n;
        o4.v[e] = gru_gate(ar.v[e], az.v[e], anx.v[e], anh.v[e], hv.v[e], r, z, n);
        r4.v[e] = r;
        z4.v[e] = z;
        n4.v[e] = n;
    }
    stv<V>(y + row * ldy + u, o4);
    stv<V>(a, r4);
    stv<V>(a + H, z4);
    stv<V>(a + 2 * H, n4);
}

// transposed (I + A) aggregate of dm for row r, unit u (gm_gru_cell_bwd): members of r's node in ascending id,
// each scaled by 1 / |{n} U nbr(n)| for mean (k_lstm_cell_bwd's loop)
template <int V>
__device__ __forceinline__ void gru_dm_add(const gm_gru_bwd_args& a, long long r, int u, Vec<V>& g) {
    const int N = a.n_nodes;
    const long long gr = r / N;
    const int n = (int)(r - gr * N);
    int mem[MAXDEG + 1];
    const int cnt = members(a.nbr + r * a.deg, a.deg, n, mem);
    for (int q = 0; q < cnt; q++) {
        Vec<V> v = ldv<V>(a.dm + (gr * N + mem[q]) * a.ld_dm + u);
        if (a.mean) {
            const int32_t* nbm = a.nbr + (gr * N + mem[q]) * a.deg;
            int cm = 1;
            for (int k = 0; k < a.deg; k++) cm += nbm[k] >= 0;
            const float f = 1.0f / (float)cm;
#pragma unroll
            for (int e = 0; e < V; e++) v.v[e] = v.v[e] * f;
        }
#pragma unroll
        for (int e = 0; e < V; e++) g.v[e] += v.v[e];
    }
}

// GRU cell backward with its gradient sources summed on the fly (gm_gru_cell_bwd), the counterpart of
// k_lstm_cell_bwd / k_lstm_cell_bwd4. Thread (rl, uv) of a block of RL x H / V threads owns V consecutive units
// of the rows r0 + rl, r0 + rl + RL, ... of the block's rows_per_block rows (V = 4: 16-byte loads and stores,
// every ld and base 16-byte aligned). Rows and columns are indexed in 32 bits relative to the block's first row
// (the host checks rows_per_block * ld < 2^31); only the dm gather reaches other blocks' rows. Bias partials:
// the RL row lanes combined in LDS in a fixed order; max |dgates| per wave, then over the block's waves
// (blockDim.x is a multiple of 64 for every accepted H).
template <int V>
__global__ __launch_bounds__(V == 4 ? 256 : 1024) void k_gru_cell_bwd(gm_gru_bwd_args a, unsigned* sc_slot,
                                                                      unsigned* max_slot) {
    constexpr int TPB = V == 4 ? 256 : 1024;
    __shared__ __align__(16) float red[4][TPB * V];
    __shared__ float wmx[TPB / 64];
    const int H = a.hidden, HV = H / V, RL = blockDim.x / HV;
    const int u = (threadIdx.x % HV) * V, rl = threadIdx.x / HV;
    const long long r0 = (long long)blockIdx.x * a.rows_per_block;
    const int nr = (int)min((long long)a.rows_per_block, (long long)a.m - r0);
    const float* act = a.act + r0 * a.ld_act;
    const float* hin = a.h + r0 * a.ld_h;
    const float* dh0 = a.dh0 ? a.dh0 + r0 * a.ld_dh0 : nullptr;
    const float* dh1 = a.dh1 ? a.dh1 + r0 * a.ld_dh1 : nullptr;
    const float* dh2 = a.dh2 ? a.dh2 + r0 * a.ld_dh2 : nullptr;
    const float* dhe = a.dh_ext ? a.dh_ext + r0 * a.ld_ext : nullptr;
    float* dgb = a.dgates + r0 * a.ld_dg;
    float* dhd = a.dh_dir ? a.dh_dir + r0 * a.ld_dhd : nullptr;
    const int ld_act = (int)a.ld_act, ld_h = (int)a.ld_h, ld_dh0 = (int)a.ld_dh0, ld_dh1 = (int)a.ld_dh1,
              ld_dh2 = (int)a.ld_dh2, ld_ext = (int)a.ld_ext, ld_dg = (int)a.ld_dg, ld_dhd = (int)a.ld_dhd;
    Vec<V> p[4];
#pragma unroll
    for (int k = 0; k < 4; k++) p[k] = zerov<V>();
    float mx = 0.f;
    for (int i = rl; i < nr; i += RL) {
        const float* ar = act + i * ld_act + u;
        const Vec<V> rv = ldv<V>(ar), zv = ldv<V>(ar + H), nv = ldv<V>(ar + 2 * H), av = ldv<V>(ar + 3 * H);
        const Vec<V> hv = ldv<V>(hin + i * ld_h + u);
        Vec<V> g = zerov<V>();
        auto add = [&g](const Vec<V>& s) {
#pragma unroll
            for (int e = 0; e < V; e++) g.v[e] += s.v[e];
        };
        if (dh0) add(ldv<V>(dh0 + i * ld_dh0 + u));
        if (dh1) add(ldv<V>(dh1 + i * ld_dh1 + u));
        if (dh2) add(ldv<V>(dh2 + i * ld_dh2 + u));
        if (a.dm) gru_dm_add<V>(a, r0 + i, u, g);
        if (dhe && (!a.ext_mask || !a.ext_mask[(r0 + i) / a.rows_per_sample])) add(ldv<V>(dhe + i * ld_ext + u));
        Vec<V> o0, o1, o2, o3, od;
#pragma unroll
        for (int e = 0; e < V; e++) {
            const float r = rv.v[e], z = zv.v[e], n = nv.v[e];
            const float dan = g.v[e] * (1.f - z) * (1.f - n * n);
            o0.v[e] = dan * av.v[e] * r * (1.f - r);
            o1.v[e] = g.v[e] * (hv.v[e] - n) * z * (1.f - z);
            o2.v[e] = dan;
            o3.v[e] = dan * r;
            od.v[e] = g.v[e] * z;
            mx = fmaxf(mx, fmaxf(fmaxf(fabsf(o0.v[e]), fabsf(o1.v[e])), fmaxf(fabsf(o2.v[e]), fabsf(o3.v[e]))));
        }
        float* dg = dgb + i * ld_dg + u;
        stv<V>(dg, o0);
        stv<V>(dg + H, o1);
        stv<V>(dg + 2 * H, o2);
        stv<V>(dg + 3 * H, o3);
        if (dhd) stv<V>(dhd + i * ld_dhd + u, od);
#pragma unroll
        for (int e = 0; e < V; e++) {
            p[0].v[e] += o0.v[e];
            p[1].v[e] += o1.v[e];
            p[2].v[e] += o2.v[e];
            p[3].v[e] += o3.v[e];
        }
    }
    if (a.bias_part) {
#pragma unroll
        for (int k = 0; k < 4; k++) stv<V>(&red[k][threadIdx.x * V], p[k]);
        __syncthreads();
        if (rl == 0) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                Vec<V> s = ldv<V>(&red[k][threadIdx.x * V]);
                for (int l = 1; l < RL; l++) {
                    const Vec<V> o = ldv<V>(&red[k][(l * HV + threadIdx.x) * V]);
#pragma unroll
                    for (int e = 0; e < V; e++) s.v[e] += o.v[e];
                }
                stv<V>(a.bias_part + (long long)blockIdx.x * 4 * H + k * H + u, s);
            }
        }
    }
    if (sc_slot || max_slot) {
        mx = gm_wave_max(mx);
        if ((threadIdx.x & 63) == 0) wmx[threadIdx.x >> 6] = mx;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < (int)(blockDim.x >> 6); w++) mx = fmaxf(mx, wmx[w]);
            if (sc_slot) gm_amax_publish(sc_slot, mx);
            if (max_slot) gm_amax_publish(max_slot, mx);
        }
    }
}
}  // namespace

static int lnlstm_fwd(const char* name, const float* gi, int64_t ldgi, const float* gh, int64_t ldgh, const float* c,
                      int64_t ldc, const LnLstmP& p, int32_t m, int32_t H, float eps, float* h1, int64_t ldh, float* c1,
                      int64_t ldc1, float* stats, void* stream) {
    if (!gi || !gh || !c || !h1 || !c1 || !p.gi_w || !p.gi_b || !p.gh_w || !p.gh_b || !p.bias || !p.lc_w || !p.lc_b ||
        m <= 0 || H <= 0 || H > 512 || ldgi < 4 * (int64_t)H || ldgh < 4 * (int64_t)H || ldc < H || ldh < H || ldc1 < H)
        return gm_fail(GM_ERR_INVALID_ARG, std::string(name) + ": bad arguments (H <= 512, gate rows >= 4H)");
    const dim3 grid((m + 3) / 4), blk(256);
    hipStream_t st = (hipStream_t)stream;
#define GM_LN(U)                                                                                                    \
    do {                                                                                                            \
        g_last_lnlstm_pw = "k_lnlstm_pw<" #U ">";                                                                   \
        hipLaunchKernelGGL(k_lnlstm_pw<U>, grid, blk, 0, st, gi, (long long)ldgi, gh, (long long)ldgh, c,           \
                           (long long)ldc, p, m, H, eps, h1, (long long)ldh, c1, (long long)ldc1, stats);           \
    } while (0)
    if (H <= 64)
        GM_LN(1);
    else if (H <= 128)
        GM_LN(2);
    else if (H <= 256)
        GM_LN(4);
    else
        GM_LN(8);
#undef GM_LN
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return gm_fail(GM_ERR_HIP, std::string(name) + ": " + hipGetErrorString(e));
    return GM_OK;
}

extern "C" int gm_lnlstm_pointwise(const float* g, int64_t ldg, const float* c, int64_t ldc, const float* ln_in_w,
                                   const float* ln_in_b, const float* ln_hid_w, const float* ln_hid_b,
                                   const float* bias, const float* ln_cell_w, const float* ln_cell_b, int32_t m,
                                   int32_t H, float eps, float* h1, int64_t ldh, float* c1, int64_t ldc1,
                                   void* stream) {
    if (!g || ldg < 8 * (int64_t)H)
        return gm_fail(GM_ERR_INVALID_ARG, "gm_lnlstm_pointwise: bad arguments (H <= 512, ldg >= 8H)");
    LnLstmP p{ln_in_w, ln_in_b, ln_hid_w, ln_hid_b, bias, ln_cell_w, ln_cell_b};
    return lnlstm_fwd("gm_lnlstm_pointwise", g, ldg, g + 4 * (int64_t)H, ldg, c, ldc, p, m, H, eps, h1, ldh, c1, ldc1,
                      nullptr, stream);
}

extern "C" int gm_lnlstm_fwd(const float* gi, int64_t ldgi, const float* gh, int64_t ldgh, const float* c,
                             int64_t ldc, const float* ln_in_w, const float* ln_in_b, const float* ln_hid_w,
                             const float* ln_hid_b, const float* bias, const float* ln_cell_w, const float* ln_cell_b,
                             int32_t m, int32_t H, float eps, float* h1, int64_t ldh, float* c1, int64_t ldc1,
                             float* stats, void* stream) {
    if (!stats) return gm_fail(GM_ERR_INVALID_ARG, "gm_lnlstm_fwd: stats is required");
    LnLstmP p{ln_in_w, ln_in_b, ln_hid_w, ln_hid_b, bias, ln_cell_w, ln_cell_b};
    return lnlstm_fwd("gm_lnlstm_fwd", gi, ldgi, gh, ldgh, c, ldc, p, m, H, eps, h1, ldh, c1, ldc1, stats, stream);
}

extern "C" int gm_lnlstm_bwd(const float* gi, int64_t ldgi, const float* gh, int64_t ldgh, const float* c,
                             int64_t ldc, const float* ln_in_w, const float* ln_in_b, const float* ln_hid_w,
                             const float* ln_hid_b, const float* bias, const float* ln_cell_w, const float* ln_cell_b,
                             const float* stats, const float* dh1, int64_t lddh, const float* dc1, int64_t lddc,
                             int32_t m, int32_t H, int32_t rows_per_wave, float* dgi, int64_t lddgi, float* dgh,
                             int64_t lddgh, float* dc, int64_t lddco, float* part, void* stream) {
    if (!gi || !gh || !c || !stats || !dgi || !dgh || !dc || !part || !ln_in_w || !ln_in_b || !ln_hid_w || !ln_hid_b ||
        !bias || !ln_cell_w || !ln_cell_b || (!dh1 && !dc1) || m <= 0 || H <= 0 || H > 512 || rows_per_wave <= 0 ||
        ldgi < 4 * (int64_t)H || ldgh < 4 * (int64_t)H || lddgi < 4 * (int64_t)H || lddgh < 4 * (int64_t)H ||
        ldc < H || lddco < H || (dh1 && lddh < H) || (dc1 && lddc < H))
        return gm_fail(GM_ERR_INVALID_ARG, "gm_lnlstm_bwd: bad arguments (H <= 512, gate rows >= 4H)");
    LnLstmP p{ln_in_w, ln_in_b, ln_hid_w, ln_hid_b, bias, ln_cell_w, ln_cell_b};
    const long long waves = ((long long)m + rows_per_wave - 1) / rows_per_wave;
    const dim3 grid((unsigned)((waves + 3) / 4)), blk(256);
    hipStream_t st = (hipStream_t)stream;
#define GM_LNB(U)                                                                                                     \
    do {                                                                                                              \
        GM_RAN("k_lnlstm_bwd<" #U ">");                                                                               \
        hipLaunchKernelGGL(k_lnlstm_bwd<U>, grid, blk, 0, st, gi, (long long)ldgi, gh, (long long)ldgh, c,            \
                           (long long)ldc, p, stats, dh1, (long long)lddh, dc1, (long long)lddc, m, H, rows_per_wave, \
                           dgi, (long long)lddgi, dgh, (long long)lddgh, dc, (long long)lddco, part);                 \
    } while (0)
    if (H <= 64)
        GM_LNB(1);
    else if (H <= 128)
        GM_LNB(2);
    else if (H <= 256)
        GM_LNB(4);
    else
        GM_LNB(8);
#undef GM_LNB
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return gm_fail(GM_ERR_HIP, std::string("gm_lnlstm_bwd: ") + hipGetErrorString(e));
    return GM_OK;
}

extern "C" int gm_lnlstm_cell_bwd(const gm_lnlstm_cell_bwd_args* a, void* stream) {
    if (!a || !a->gi || !a->gh || !a->c_in || !a->stats || !a->dgi || !a->dgh || !a->ln_in_w || !a->ln_in_b ||
        !a->ln_hid_w || !a->ln_hid_b || !a->bias || !a->ln_cell_w || !a->ln_cell_b || a->m <= 0 || a->hidden <= 0 ||
        !(a->eps >= 0.f) || (a->dm && (!a->nbr || a->n_nodes <= 0 || a->deg < 0 || a->deg > MAXDEG)) ||
        (a->ext_mask && a->rows_per_sample <= 0) || a->rows_per_wave < 0)
        return gm_fail(GM_ERR_INVALID_ARG, "gm_lnlstm_cell_bwd: bad arguments");
    const int H = a->hidden;
    if (H > 512) return gm_fail(GM_ERR_UNSUPPORTED, "gm_lnlstm_cell_bwd: hidden must be at most 512");
    const int64_t H4 = 4 * (int64_t)H;
    if (a->ld_gi < H4 || a->ld_gh < H4 || a->ld_dgi < H4 || a->ld_dgh < H4 || a->ld_cin < H ||
        (a->dh0 && a->ld_dh0 < H) || (a->dh1 && a->ld_dh1 < H) || (a->dm && a->ld_dm < H) ||
        (a->dh_ext && a->ld_ext < H) || (a->dc_ext && a->ld_dcext < H) || (a->dc && a->ld_dc < H) ||
        (a->dc_out && a->ld_dco < H))
        return gm_fail(GM_ERR_INVALID_ARG, "gm_lnlstm_cell_bwd: row strides (gate rows >= 4H, state rows >= H)");
    hipStream_t st = (hipStream_t)stream;
    gm_lnlstm_cell_bwd_args b = *a;
    if (b.rows_per_wave <= 0) b.rows_per_wave = 8;
    if (!b.ext_mask) b.rows_per_sample = 1;
    for (float* s : {b.dgi_scale, b.dgh_scale})
        if (s && hipMemsetAsync(s, 0, sizeof(float), st) != hipSuccess)
            return gm_fail(GM_ERR_HIP, "gm_lnlstm_cell_bwd: memset");
    LnLstmP p{b.ln_in_w, b.ln_in_b, b.ln_hid_w, b.ln_hid_b, b.bias, b.ln_cell_w, b.ln_cell_b};
    const long long waves = ((long long)b.m + b.rows_per_wave - 1) / b.rows_per_wave;
    const dim3 grid((unsigned)((waves + 3) / 4)), blk(256);
    unsigned* sci = reinterpret_cast<unsigned*>(b.dgi_scale);
    unsigned* sch = reinterpret_cast<unsigned*>(b.dgh_scale);
    GM_RAN("k_lnlstm_cell_bwd");
    if (H <= 64)
        hipLaunchKernelGGL(k_lnlstm_cell_bwd<1>, grid, blk, 0, st, b, p, sci, sch);
    else if (H <= 128)
        hipLaunchKernelGGL(k_lnlstm_cell_bwd<2>, grid, blk, 0, st, b, p, sci, sch);
    else if (H <= 256)
        hipLaunchKernelGGL(k_lnlstm_cell_bwd<4>, grid, blk, 0, st, b, p, sci, sch);
    else
        hipLaunchKernelGGL(k_lnlstm_cell_bwd<8>, grid, blk, 0, st, b, p, sci, sch);
    int rc = launched();
    if (rc == GM_OK && b.dgi_scale) rc = gm_absmax_finish(b.dgi_scale, stream);
    if (rc == GM_OK && b.dgh_scale) rc = gm_absmax_finish(b.dgh_scale, stream);
    return rc;
}

extern "C" int gm_gru_pointwise(const float* gi, int64_t ldgi, const float* gh, int64_t ldgh, const float* h,
                                int64_t ldh, int32_t m, int32_t H, float* h1, int64_t ldh1, void* stream) {
    if (!gi || !gh || !h || !h1 || m <= 0 || H <= 0 || ldgi < 3 * (int64_t)H || ldgh < 3 * (int64_t)H || ldh < H ||
        ldh1 < H)
        return gm_fail(GM_ERR_INVALID_ARG, "gm_gru_pointwise: bad arguments (gate rows >= 3H)");
    const long long n = (long long)m * H;
    GM_RAN("k_gru_pw");
    hipLaunchKernelGGL(k_gru_pw, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gi,
                       (long long)ldgi, gh, (long long)ldgh, h, (long long)ldh, m, H, h1, (long long)ldh1);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return gm_fail(GM_ERR_HIP, std::string("gm_gru_pointwise: ") + hipGetErrorString(e));
    return GM_OK;
}

extern "C" int gm_gru_bwd(const float* gi, int64_t ldgi, const float* gh, int64_t ldgh, const float* h, int64_t ldh,
                          const float* dh1, int64_t lddh1, int32_t m, int32_t H, float* dgi, int64_t lddgi, float* dgh,
                          int64_t lddgh, float* dh, int64_t lddh, void* stream) {
    if (!gi || !gh || !h || !dh1 || !dgi || !dgh || !dh || m <= 0 || H <= 0 || ldgi < 3 * (int64_t)H ||
        ldgh < 3 * (int64_t)H || ldh < H || lddh1 < H || lddgi < 3 * (int64_t)H || lddgh < 3 * (int64_t)H || lddh < H)
        return gm_fail(GM_ERR_INVALID_ARG, "gm_gru_bwd: bad arguments (gate rows >= 3H)");
    const long long n = (long long)m * H;
    GM_RAN("k_gru_bwd");
    hipLaunchKernelGGL(k_gru_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gi,
                       (long long)ldgi, gh, (long long)ldgh, h, (long long)ldh, dh1, (long long)lddh1, m, H, dgi,
                       (long long)lddgi, dgh, (long long)lddgh, dh, (long long)lddh);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return gm_fail(GM_ERR_HIP, std::string("gm_gru_bwd: ") + hipGetErrorString(e));
    return GM_OK;
}

extern "C" int gm_gru_cell_fwd(float* p, int64_t ldp, const float* h, int64_t ldh, int32_t m, int32_t H, float* h1,
                               int64_t ldh1, void* stream) {
    if (!p || !h || !h1 || m <= 0 || H <= 0 || ldp < 4 * (int64_t)H || ldh < H || ldh1 < H)
        return gm_fail(GM_ERR_INVALID_ARG, "gm_gru_cell_fwd: bad arguments (gate rows >= 4H)");
    auto a16 = [](const void* q, long long ld) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0 && ld % 4 == 0; };
    const bool vec = H % 4 == 0 && a16(p, ldp) && a16(h, ldh) && a16(h1, ldh1);
    const long long n = (long long)m * (vec ? H / 4 : H);
    const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
    hipStream_t st = (hipStream_t)stream;
    if (vec) {
        GM_RAN("k_gru_cell_fwd<4>");
        hipLaunchKernelGGL(k_gru_cell_fwd<4>, grid, blk, 0, st, p, (long long)ldp, h, (long long)ldh, m, H, h1,
                           (long long)ldh1);
    } else {
        GM_RAN("k_gru_cell_fwd<1>");
        hipLaunchKernelGGL(k_gru_cell_fwd<1>, grid, blk, 0, st, p, (long long)ldp, h, (long long)ldh, m, H, h1,
                           (long long)ldh1);
    }
    return launched();
}

extern "C" int gm_gru_cell_bwd(const gm_gru_bwd_args* a, void* stream) {
    if (!a || !a->act || !a->h || !a->dgates || a->m <= 0 || a->hidden <= 0 ||
        (a->dm && (!a->nbr || a->n_nodes <= 0 || a->deg < 0 || a->deg > MAXDEG)) ||
        (a->ext_mask && a->rows_per_sample <= 0) || (a->bias_part && a->rows_per_block <= 0))
        return gm_fail(GM_ERR_INVALID_ARG, "gm_gru_cell_bwd: bad arguments");
    const int H = a->hidden;
    if (!((H <= 256 && 256 % H == 0) || (H % 64 == 0 && H <= 1024)))
        return gm_fail(GM_ERR_UNSUPPORTED, "gm_gru_cell_bwd: hidden must divide 256 or be a multiple of 64 up to 1024");
    hipStream_t st = (hipStream_t)stream;
    gm_gru_bwd_args b = *a;
    if (b.rows_per_block <= 0) b.rows_per_block = 64;
    // the kernels index a block's rows in 32 bits
    long long ldmax = std::max((long long)b.ld_act, (long long)b.ld_dg);
    for (long long ld : {(long long)b.ld_h, (long long)(b.dh0 ? b.ld_dh0 : 0), (long long)(b.dh1 ? b.ld_dh1 : 0),
                         (long long)(b.dh2 ? b.ld_dh2 : 0), (long long)(b.dh_ext ? b.ld_ext : 0),
                         (long long)(b.dh_dir ? b.ld_dhd : 0)})
        ldmax = std::max(ldmax, ld);
    if (b.ld_act < 4 * (int64_t)H || b.ld_dg < 4 * (int64_t)H || b.ld_h < H ||
        (ldmax + 4 * (long long)H) * b.rows_per_block >= (1LL << 31))
        return gm_fail(GM_ERR_INVALID_ARG, "gm_gru_cell_bwd: row strides (>= 4H gate rows; rows_per_block * ld < 2^31)");
    if (b.dg_scale && hipMemsetAsync(b.dg_scale, 0, sizeof(float), st) != hipSuccess)
        return gm_fail(GM_ERR_HIP, "gm_gru_cell_bwd: memset");
    const long long nb = ((long long)b.m + b.rows_per_block - 1) / b.rows_per_block;
    auto a16 = [](const void* p, long long ld) { return !p || ((reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0); };
    const bool vec = H % 4 == 0 && H / 4 <= 256 && ((256 / (H / 4)) * (H / 4)) % 64 == 0 && a16(b.act, b.ld_act) &&
                     a16(b.h, b.ld_h) && a16(b.dh0, b.ld_dh0) && a16(b.dh1, b.ld_dh1) && a16(b.dh2, b.ld_dh2) &&
                     a16(b.dm, b.ld_dm) && a16(b.dh_ext, b.ld_ext) && a16(b.dgates, b.ld_dg) &&
                     a16(b.dh_dir, b.ld_dhd) && a16(b.bias_part, 4);
    if (vec) {
        const int rl4 = 256 / (H / 4);
        GM_RAN("k_gru_cell_bwd<4>");
        hipLaunchKernelGGL(k_gru_cell_bwd<4>, dim3((unsigned)nb), dim3(rl4 * (H / 4)), 0, st, b,
                           reinterpret_cast<unsigned*>(b.dg_scale), reinterpret_cast<unsigned*>(b.dg_max));
    } else {
        const int RL = H >= 256 ? 1 : 256 / H;
        GM_RAN("k_gru_cell_bwd<1>");
        hipLaunchKernelGGL(k_gru_cell_bwd<1>, dim3((unsigned)nb), dim3(H * RL), 0, st, b,
                           reinterpret_cast<unsigned*>(b.dg_scale), reinterpret_cast<unsigned*>(b.dg_max));
    }
    int rc = launched();
    if (rc == GM_OK && b.dg_scale) rc = gm_absmax_finish(b.dg_scale, stream);
    return rc;
}

// ---- per-step mean squared error of the SL unroll (src/sl.py:396-400: mse_loss(pred_all, targets_all) after
// every unroll step, averaged over the steps) ----
// pred [L][n] (every step's prediction), tgt [n] (the same target at every step), n % 4 == 0, 16-byte
// bases. Block b owns float4 indices [b * 256 * V, (b + 1) * 256 * V) of a step; its target elements are loaded
// once and stay in registers while the block walks the L steps (the target is not re-read per step).
namespace {
constexpr int MSE_V = 4;

__global__ __launch_bounds__(256) void k_step_mse_fwd(const float4* __restrict__ pred, const float4* __restrict__ tgt,
                                                      long long n4, int L, float* __restrict__ part) {
    __shared__ float wsum[4];
    const long long base = (long long)blockIdx.x * (256 * MSE_V) + threadIdx.x;
    float4 t[MSE_V];
#pragma unroll
    for (int v = 0; v < MSE_V; v++) {
        const long long i = base + (long long)v * 256;
        t[v] = i < n4 ? tgt[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int l = 0; l < L; l++) {
        const float4* pl = pred + (long long)l * n4;
        float4 p[MSE_V];
#pragma unroll
        for (int v = 0; v < MSE_V; v++) {
            const long long i = base + (long long)v * 256;
            p[v] = i < n4 ? pl[i] : t[v];  // past the end: d = 0
        }
        float s = 0.f;
#pragma unroll
        for (int v = 0; v < MSE_V; v++) {
            const float dx = p[v].x - t[v].x, dy = p[v].y - t[v].y, dz = p[v].z - t[v].z, dw = p[v].w - t[v].w;
            s = fmaf(dx, dx, s);
            s = fmaf(dy, dy, s);
            s = fmaf(dz, dz, s);
            s = fmaf(dw, dw, s);
        }
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) part[(long long)l * gridDim.x + blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        __syncthreads();
    }
}

// grad[l][i] = (pred[l][i] - tgt[i]) * (g[l] * two_over_n): torch's d * (g * (2 / n)) in fp32, element for element
__global__ __launch_bounds__(256) void k_step_mse_bwd(const float4* __restrict__ pred, const float4* __restrict__ tgt,
                                                      long long n4, int L, const float* __restrict__ g,
                                                      float two_over_n, float4* __restrict__ grad) {
    const long long base = (long long)blockIdx.x * (256 * MSE_V) + threadIdx.x;
    float4 t[MSE_V];
#pragma unroll
    for (int v = 0; v < MSE_V; v++) {
        const long long i = base + (long long)v * 256;
        t[v] = i < n4 ? tgt[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int l = 0; l < L; l++) {
        const float s = g[l] * two_over_n;
        const float4* pl = pred + (long long)l * n4;
        float4* gl = grad + (long long)l * n4;
        float4 p[MSE_V];
#pragma unroll
        for (int v = 0; v < MSE_V; v++) {
            const long long i = base + (long long)v * 256;
            p[v] = i < n4 ? pl[i] : t[v];
        }
#pragma unroll
        for (int v = 0; v < MSE_V; v++) {
            const long long i = base + (long long)v * 256;
            if (i < n4)
                gl[i] = make_float4((p[v].x - t[v].x) * s, (p[v].y - t[v].y) * s, (p[v].z - t[v].z) * s,
                                    (p[v].w - t[v].w) * s);
        }
    }
}

bool mse_args_ok(const float* pred, const float* tgt, int64_t n, int32_t L) {
    auto a16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    return pred && tgt && n > 0 && n % 4 == 0 && L > 0 && a16(pred) && a16(tgt) && n / 4 <= (1ll << 40);
}
}  // namespace

extern "C" int32_t gm_step_mse_blocks(int64_t n) {
    return n > 0 ? (int32_t)((n / 4 + 256 * MSE_V - 1) / (256 * MSE_V)) : 0;
}

extern "C" int gm_step_mse(const float* pred, const float* tgt, int64_t n, int32_t L, float* part, void* stream) {
    if (!mse_args_ok(pred, tgt, n, L) || !part)
        return gm_fail(GM_ERR_INVALID_ARG, "gm_step_mse: bad arguments (n % 4 == 0, 16-byte pred / tgt)");
    const int nb = gm_step_mse_blocks(n);
    hipLaunchKernelGGL(k_step_mse_fwd, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(pred), reinterpret_cast<const float4*>(tgt), (long long)(n / 4),
                       L, part);
    return launched();
}

extern "C" int gm_step_mse_bwd(const float* pred, const float* tgt, int64_t n, int32_t L, const float* g,
                               float two_over_n, float* grad, void* stream) {
    if (!mse_args_ok(pred, tgt, n, L) || !g || !grad || (reinterpret_cast<uintptr_t>(grad) & 15))
        return gm_fail(GM_ERR_INVALID_ARG, "gm_step_mse_bwd: bad arguments (n % 4 == 0, 16-byte pred / tgt / grad)");
    const int nb = gm_step_mse_blocks(n);
    hipLaunchKernelGGL(k_step_mse_bwd, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(pred), reinterpret_cast<const float4*>(tgt), (long long)(n / 4),
                       L, g, two_over_n, reinterpret_cast<float4*>(grad));
    return launched();
}

// ---- NetMon aux head: its narrow second layer fused with the MSE (src/main.py:586-594, 868-875: MLP(S, [S, n_aux],
// activation_on_output=False) on the new node state against get_node_aux, F.mse_loss) ----
// Forward: res[r][a] = (b2[a] + sum_c y[r][c] w2[a][c]) - tgt[r][a], the c sum one fmaf chain in ascending c, so the
// layer's [rows][n_out] output is never written and read back. A block owns rpb <= 64 rows and walks the K = cols
// contraction in 32-column chunks staged in LDS (rows padded to 33 floats: lane a reads bank (a + c) % 32): lane
// (rl, al) of the 8 x 32 block owns rows rl + 8 i and outputs al + 32 k, 8 x 4 accumulators with static indices.
// Backward: g = s (res w2) (leaky mask of y from its sign bits) with 4 columns per thread as k_qhead_bwd4, the
// block's res rows in LDS; W2's gradient s res^T y is a weight-gradient GEMM of the caller (gm_gemm_x3_wgrad).
namespace {
constexpr int AUX_RPB = 64;   // most rows per block (8 per row lane)
constexpr int AUX_NMAX = 128;  // most outputs (4 per lane)
constexpr int AUX_LD = 33;     // LDS row of a 32-column chunk

__global__ __launch_bounds__(256) void k_aux_head_mse(const float* __restrict__ y, long long ldy, long long rows,
                                                      int cols, const float* __restrict__ w2, long long ldw,
                                                      const float* __restrict__ b2, int n_out,
                                                      const float* __restrict__ tgt, long long ldt,
                                                      float* __restrict__ res, long long ldr, float* __restrict__ part,
                                                      int rpb, unsigned* __restrict__ amax,
                                                      unsigned* __restrict__ y_amax) {
    __shared__ float ys[AUX_RPB * AUX_LD];
    __shared__ float ws[AUX_NMAX * AUX_LD];
    __shared__ float wsum[4], wmx[4], wymx[4];
    const int al = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const long long r0 = (long long)blockIdx.x * rpb;
    const int nr = (int)min((long long)rpb, rows - r0);
    const int NA = (n_out + 31) >> 5, RI = (rpb + 7) >> 3;
    float acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int k = 0; k < 4; k++) acc[i][k] = 0.f;
    float ymx = 0.f;
    for (int c0 = 0; c0 < cols; c0 += 32) {
        for (int i = threadIdx.x; i < rpb * 8; i += 256) {
            const int r = i >> 3, q = i & 7;
            const float4 v = *reinterpret_cast<const float4*>(y + (r0 + min(r, nr - 1)) * ldy + c0 + 4 * q);
            ymx = fmaxf(fmaxf(ymx, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
            float* d = ys + r * AUX_LD + 4 * q;
            d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        }
        for (int i = threadIdx.x; i < n_out * 8; i += 256) {
            const int a = i >> 3, q = i & 7;
            const float4 v = *reinterpret_cast<const float4*>(w2 + a * ldw + c0 + 4 * q);
            float* d = ws + a * AUX_LD + 4 * q;
            d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        }
        __syncthreads();
#pragma unroll 4
        for (int c = 0; c < 32; c++) {
            float w[4];
#pragma unroll
            for (int k = 0; k < 4; k++) w[k] = k < NA ? ws[(al + 32 * k) * AUX_LD + c] : 0.f;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                if (i < RI) {
                    const float yv = ys[(rl + 8 * i) * AUX_LD + c];
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (k < NA) acc[i][k] = fmaf(yv, w[k], acc[i][k]);
                }
            }
        }
        __syncthreads();
    }
    float sq = 0.f, mx = 0.f;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int r = rl + 8 * i;
        if (r < nr) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int a = al + 32 * k;
                if (a < n_out) {
                    const float v = (b2[a] + acc[i][k]) - tgt[(r0 + r) * ldt + a];
                    res[(r0 + r) * ldr + a] = v;
                    sq = fmaf(v, v, sq);
                    mx = fmaxf(mx, fabsf(v));
                }
            }
        }
    }
    // the block's sum in a fixed order: lane sums, the wave's xor tree, then (w0 + w1) + (w2 + w3)
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
    mx = gm_wave_max(mx);
    ymx = gm_wave_max(ymx);
    if ((threadIdx.x & 63) == 0) {
        wsum[threadIdx.x >> 6] = sq;
        wmx[threadIdx.x >> 6] = mx;
        wymx[threadIdx.x >> 6] = ymx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        if (amax) gm_amax_publish(amax, fmaxf(fmaxf(wmx[0], wmx[1]), fmaxf(wmx[2], wmx[3])));
        if (y_amax) gm_amax_publish(y_amax, fmaxf(fmaxf(wymx[0], wymx[1]), fmaxf(wymx[2], wymx[3])));
    }
}

__global__ __launch_bounds__(256) void k_aux_head_mse_bwd(const float* __restrict__ res, long long ldr, int n_out,
                                                          const float* __restrict__ w2, long long ldw,
                                                          const unsigned* __restrict__ bits, long long ldm,
                                                          long long rows, int cols, float scale,
                                                          const float* __restrict__ scale_dev, float* __restrict__ g,
                                                          long long ldg, float* __restrict__ part_b1,
                                                          float* __restrict__ part_b2, int rpb,
                                                          unsigned* __restrict__ amax) {
    __shared__ float rs[AUX_RPB * AUX_NMAX];  // the block's res rows, [row][n_out]
    __shared__ float4 red[256];
    __shared__ float wmx[4];
    const float s = scale * (scale_dev ? *scale_dev : 1.f);
    const long long r0 = (long long)blockIdx.x * rpb;
    const int nr = (int)min((long long)rpb, rows - r0);
    for (int i = threadIdx.x; i < nr * n_out; i += 256) rs[i] = res[(r0 + i / n_out) * ldr + i % n_out];
    __syncthreads();
    const int C4 = cols >> 2, RL = 256 / C4;
    const bool active = (int)threadIdx.x < RL * C4;
    const int c4 = threadIdx.x % C4, rl = threadIdx.x / C4, c = 4 * c4;
    float4 pb = make_float4(0.f, 0.f, 0.f, 0.f);
    float mx = 0.f;
    constexpr int U = 4;
    if (active) {
        for (int rb = rl; rb < nr; rb += U * RL) {
            float4 acc[U];
            int ro[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                ro[u] = min(rb + u * RL, nr - 1) * n_out;
            }
            for (int a = 0; a < n_out; a++) {
                const float4 w = *reinterpret_cast<const float4*>(w2 + a * ldw + c);
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const float rv = rs[ro[u] + a];
                    acc[u].x = fmaf(rv, w.x, acc[u].x);
                    acc[u].y = fmaf(rv, w.y, acc[u].y);
                    acc[u].z = fmaf(rv, w.z, acc[u].z);
                    acc[u].w = fmaf(rv, w.w, acc[u].w);
                }
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int r = rb + u * RL;
                if (r >= nr) break;
                float4 v = make_float4(s * acc[u].x, s * acc[u].y, s * acc[u].z, s * acc[u].w);
                if (bits) {  // bit set: y > 0; clear: the leaky slope
                    const unsigned m = bits[(r0 + r) * ldm + (c >> 5)] >> (c & 31);
                    if (!(m & 1u)) v.x *= 0.01f;
                    if (!(m & 2u)) v.y *= 0.01f;
                    if (!(m & 4u)) v.z *= 0.01f;
                    if (!(m & 8u)) v.w *= 0.01f;
                }
                *reinterpret_cast<float4*>(g + (r0 + r) * ldg + c) = v;
                pb.x += v.x;
                pb.y += v.y;
                pb.z += v.z;
                pb.w += v.w;
                mx = fmaxf(fmaxf(mx, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
            }
        }
    }
    red[threadIdx.x] = pb;
    mx = gm_wave_max(mx);
    if ((threadIdx.x & 63) == 0) wmx[threadIdx.x >> 6] = mx;
    __syncthreads();
    if ((int)threadIdx.x < C4) {  // the row lanes' column sums in lane order
        float4 sm = red[threadIdx.x];
        for (int l = 1; l < RL; l++) {
            const float4 o = red[l * C4 + threadIdx.x];
            sm.x += o.x;
            sm.y += o.y;
            sm.z += o.z;
            sm.w += o.w;
        }
        *reinterpret_cast<float4*>(part_b1 + (long long)blockIdx.x * cols + c) = sm;
    }
    if ((int)threadIdx.x < n_out) {
        float sm = 0.f;
        for (int r = 0; r < nr; r++) sm += rs[r * n_out + threadIdx.x];
        part_b2[(long long)blockIdx.x * n_out + threadIdx.x] = s * sm;
    }
    if (amax && threadIdx.x == 0) gm_amax_publish(amax, fmaxf(fmaxf(wmx[0], wmx[1]), fmaxf(wmx[2], wmx[3])));
}

bool aux_a16(const void* p, long long ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0; }
bool aux_a4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
}  // namespace

extern "C" int gm_aux_head_mse(const float* y, int64_t ldy, int64_t rows, int32_t cols, const float* w2, int64_t ldw,
                               const float* b2, int32_t n_out, const float* tgt, int64_t ldt, float* res, int64_t ldr,
                               float* part, int32_t rows_per_block, float* res_amax, float* y_amax, void* stream) {
    if (!y || !w2 || !b2 || !tgt || !res || !part || rows <= 0 || cols < 32 || cols > 1024 || cols % 32 || n_out < 1 ||
        n_out > AUX_NMAX || rows_per_block < 8 || rows_per_block > AUX_RPB || rows_per_block % 8 || ldy < cols ||
        ldw < cols || ldt < n_out || ldr < n_out || !aux_a16(y, ldy) || !aux_a16(w2, ldw) || !aux_a4(b2) ||
        !aux_a4(tgt) || !aux_a4(res) || !aux_a4(part) || !aux_a4(res_amax) || !aux_a4(y_amax) ||
        (rows + rows_per_block - 1) / rows_per_block > 0x7fffffffll)
        return gm_fail(GM_ERR_INVALID_ARG,
                       "gm_aux_head_mse: bad arguments (cols % 32 == 0, cols <= 1024, 1 <= n_out <= 128, rows_per_block "
                       "a multiple of 8 up to 64, y / w2 rows 16-byte aligned)");
    const long long nb = (rows + rows_per_block - 1) / rows_per_block;
    GM_RAN("k_aux_head_mse");
    hipLaunchKernelGGL(k_aux_head_mse, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, y, (long long)ldy,
                       (long long)rows, cols, w2, (long long)ldw, b2, n_out, tgt, (long long)ldt, res, (long long)ldr,
                       part, rows_per_block, reinterpret_cast<unsigned*>(res_amax),
                       reinterpret_cast<unsigned*>(y_amax));
    return launched();
}

extern "C" int gm_aux_head_mse_bwd(const float* res, int64_t ldr, int32_t n_out, const float* w2, int64_t ldw,
                                   const uint32_t* mask_bits, int64_t ldm, int32_t act, int64_t rows, int32_t cols,
                                   float scale, const float* scale_dev, float* g, int64_t ldg, float* part_b1,
                                   float* part_b2, int32_t rows_per_block, float* g_scale, void* stream) {
    if (!res || !w2 || !g || !part_b1 || !part_b2 || rows <= 0 || cols < 32 || cols > 1024 || cols % 32 || n_out < 1 ||
        n_out > AUX_NMAX || rows_per_block < 1 || rows_per_block > AUX_RPB || ldr < n_out || ldw < cols || ldg < cols ||
        (act != 0 && act != 1) || (act == 1 && (!mask_bits || ldm < cols / 32 || !aux_a4(mask_bits))) ||
        !aux_a4(res) || !aux_a16(w2, ldw) || !aux_a16(g, ldg) || !aux_a16(part_b1, 4) || !aux_a4(part_b2) ||
        !aux_a4(scale_dev) || !aux_a4(g_scale) || (rows + rows_per_block - 1) / rows_per_block > 0x7fffffffll)
        return gm_fail(GM_ERR_INVALID_ARG,
                       "gm_aux_head_mse_bwd: bad arguments (cols % 32 == 0, cols <= 1024, 1 <= n_out <= 128, "
                       "rows_per_block <= 64, act 0 / 1 with mask_bits, w2 / g rows and part_b1 16-byte aligned)");
    hipStream_t st = (hipStream_t)stream;
    if (g_scale && hipMemsetAsync(g_scale, 0, sizeof(float), st) != hipSuccess)
        return gm_fail(GM_ERR_HIP, "gm_aux_head_mse_bwd: memset");
    const long long nb = (rows + rows_per_block - 1) / rows_per_block;
    GM_RAN("k_aux_head_mse_bwd");
    hipLaunchKernelGGL(k_aux_head_mse_bwd, dim3((unsigned)nb), dim3(256), 0, st, res, (long long)ldr, n_out, w2,
                       (long long)ldw, act ? mask_bits : nullptr, (long long)ldm, (long long)rows, cols, scale,
                       scale_dev, g, (long long)ldg, part_b1, part_b2, rows_per_block,
                       reinterpret_cast<unsigned*>(g_scale));
    int rc = launched();
    if (rc == GM_OK && g_scale) rc = gm_absmax_finish(g_scale, stream);
    return rc;
}
