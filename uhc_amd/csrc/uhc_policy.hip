// A frozen policy as a library object: raw observations -> action means, float64, without the framework (uhc/khrylib/rl/core/policy_gaussian.py:9-31,
// uhc/models/policy_mcp.py:9-37, the mean action of select_action behind ZFilter(update=False)).
//
// A policy is a list of NETS, each a chain of layers Y = act(X W^T + b): Gaussian is one net (the trunk and its linear head), MCP is P primitive nets of equal
// shape plus the composer, whose last layer is activated too, then softmax; the action mean is the composer-weighted sum of the primitives' means.
//
//   uhc_policy_layer_kernel   layer l of every net in one launch (grid z = net).  A wave owns 16 output columns and keeps the accumulators of POL_RT row tiles
//                             (64 rows) live: per k-step one coalesced 512-byte read of the packed weight serves POL_RT v_mfma_f64_16x16x4_f64.  The four
//                             waves of a workgroup take a quarter of K each and add their sums in LDS in wave order.  Bias and activation in the
//                             epilogue; the result is stored in the order the next layer reads its A operand (uhc_policy_math.h), a net's
//                             last layer row-major.  The first layer reads the caller's observations where they lie (row stride) and applies the
//                             observation filter on the way in, with the arithmetic of uhc_filter_apply; the wave of column tile 0 of net 0 writes the
//                             filtered observation out.
//   uhc_policy_combine_kernel MCP only: softmax over the composer's P outputs, mean = sum_p w_p mean_p in the order p = 0 .. P - 1.
//   uhc_policy_pack_kernel    raw nn.Linear weights ([out][in]) and biases -> packed, padded with zeros (create, set_params).
//
// So a call is depth launches (Gaussian) or depth + 1 (MCP) in a straight chain on one stream: nothing orders the layers but the stream -- no cooperative
// launch, no grid-wide barrier, no flag --, and a HIP graph captures it as a chain.  Every sum has a fixed order (k ascending within a run, the four runs
// in wave order, no atomics) and a row's result is formed from that row's data alone: two runs are bit-identical, and so is a row wherever it sits in whatever batch.
// No index is read from memory: no value in any array can send a read or a write outside the arrays.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/uhc_amd.h"  // (declares the entry points below with default visibility: the library is built -fvisibility=hidden)
#include "uhc_api_check.h"
#include "uhc_policy_math.h"

#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ != __ORDER_LITTLE_ENDIAN__
#error "uhc_policy_save / uhc_policy_load write the host's words as they lie: a little-endian host"
#endif

static_assert(UHC_ACT_NONE == UHC_POL_ACT_NONE && UHC_ACT_TANH == UHC_POL_ACT_TANH && UHC_ACT_RELU == UHC_POL_ACT_RELU &&
                  UHC_ACT_SIGMOID == UHC_POL_ACT_SIGMOID && UHC_ACT_GELU == UHC_POL_ACT_GELU,
              "the activation codes of include/uhc_amd.h are those of uhc_policy_math.h");

#define POL_RT 4     // row tiles (of 16 rows) whose accumulators a wave keeps live
#define POL_WAVES 4  // waves per workgroup: the runs K is split into; equal to POL_RT, wave w finishes row tile w
#define POL_KU 4     // k-steps whose operands are loaded ahead of their products
static_assert(POL_WAVES == POL_RT, "wave w finishes row tile w");
#define POL_MAX_DIM (1 << 20)
#define POL_MAX_NETS 1024
#define POL_MAX_LAYERS 64

typedef double pol_v4d __attribute__((ext_vector_type(4)));

// one net at one layer (device table [depth][n_nets]); offsets in doubles
struct PolDesc {
    long long w_off, b_off;  // the packed weight, the bias padded to 16
    long long in_off;        // the packed input (layers > 0)
    long long out_off;       // the packed output, or the net's row-major result when `final`
    int K, N, act, final;    // N == 0: the net has no such layer
};

// what a call hands its kernels
struct PolCall {
    const double *w, *b;
    double* x;         // the packed activations between the layers
    double* fin;       // the nets' row-major results: Gaussian -- the caller's d_mean; MCP -- the handle's
    const double* obs;
    long long obs_stride;
    double* state_out;  // or NULL
    const double* filt;  // [2][obs_dim]: mean, std + 1e-8
    int n_rows, obs_dim, filter_on, demean, destd;
    double clip;
};

struct UhcPolicy {
    int kind = 0, obs_dim = 0, act_dim = 0, max_rows = 0, n_nets = 0, depth = 0, P = 0;
    std::vector<int> n_layers, first;  // per net; first: index of its first layer in the flat (net-major) layer list
    std::vector<int> widths, acts;     // per flat layer
    std::vector<size_t> raw_w, raw_b;  // per flat layer: where W and b lie in d_raw
    std::vector<PolDesc> desc;         // [depth][n_nets]
    size_t raw_total = 0, n_packed = 0;  // doubles of d_raw; of the packed weights and biases together
    int has_filter = 0, demean = 0, destd = 0;
    double clip = 0.0, filt_n = 0.0;
    std::vector<double> filt_mean, filt_S;
    double *d_raw = nullptr, *d_w = nullptr, *d_b = nullptr, *d_x = nullptr, *d_final = nullptr, *d_filt = nullptr, *d_filt_in = nullptr;
    PolDesc* d_desc = nullptr;
    int in_dim(int net, int l) const { return l == 0 ? obs_dim : widths[first[net] + l - 1]; }
};

// ------------------------------------------------------------------ raw -> packed
__global__ void __launch_bounds__(256) uhc_policy_pack_kernel(const double* __restrict__ W, const double* __restrict__ bias, int N, int K, double* __restrict__ wp,
                                                              double* __restrict__ bp) {
    const int kpad = uhc_pol_pad4(K), npad = uhc_pol_pad16(N), ksteps = kpad >> 2;
    const long long nw = (long long)npad * kpad;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < nw) {  // slot idx of the packed weight: [column tile][k-step][lane]
        const int lane = (int)(idx & 63), ks = (int)((idx >> 6) % ksteps), ct = (int)((idx >> 6) / ksteps);
        const int n = 16 * ct + uhc_pol_b_col(lane), k = uhc_pol_ab_k(lane, ks);
        wp[idx] = (n < N && k < K) ? W[(size_t)n * K + k] : 0.0;
    } else if (idx < nw + npad) {
        const int n = (int)(idx - nw);
        bp[n] = n < N ? bias[n] : 0.0;
    }
}

__global__ void __launch_bounds__(256) uhc_policy_filter_kernel(const double* __restrict__ in /* n, mean[dim], S[dim] */, int dim, double* __restrict__ filt) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= dim) return;
    const double m = in[1 + k];
    filt[k] = m;
    filt[dim + k] = uhc_pol_filter_denom(in[0], m, in[1 + dim + k]);
}

// ------------------------------------------------------------------ one layer of every net
// The four waves of a workgroup share one column tile and split K into four contiguous runs of k-steps (a function of K alone, so a row's bits do not
// depend on the batch); each keeps POL_RT row tiles' accumulators live and loads POL_KU k-steps ahead of the products that use them.  The partial sums meet in
// LDS and are added in wave order 0, 1, 2, 3; wave w then finishes row tile w: bias, activation, store.
template <bool FIRST>
__global__ void __launch_bounds__(64 * POL_WAVES) uhc_policy_layer_kernel(PolCall c, const PolDesc* __restrict__ desc) {
    __shared__ double part[POL_WAVES][POL_RT][4][64];  // [wave][row tile][register][lane]
    const PolDesc d = desc[blockIdx.z];
    const int ct = blockIdx.x;
    if (d.N == 0 || 16 * ct >= d.N) return;  // (uniform over the workgroup: before the barrier)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ntile = (c.n_rows + 15) >> 4, rt0 = blockIdx.y * POL_RT;
    const int ksteps = uhc_pol_pad4(d.K) >> 2;
    const int per = (ksteps + POL_WAVES - 1) / POL_WAVES, ks0 = wave * per, ks1 = ks0 + per < ksteps ? ks0 + per : ksteps;
    const double* __restrict__ wp = c.w + d.w_off + (size_t)ct * ksteps * 64 + lane;
    pol_v4d acc[POL_RT];
#pragma unroll
    for (int t = 0; t < POL_RT; t++) acc[t] = pol_v4d{0.0, 0.0, 0.0, 0.0};

    if (FIRST) {
        // A from the caller's rows: lane l holds X[16 rt + (l & 15)][4 ks + (l >> 4)], filtered on the way in; zero beyond the rows and beyond the width
        const bool writer = c.state_out != nullptr && blockIdx.z == 0 && ct == 0;
        long long row[POL_RT];
        bool live[POL_RT];
#pragma unroll
        for (int t = 0; t < POL_RT; t++) {
            row[t] = 16LL * (rt0 + t) + uhc_pol_a_row(lane);
            live[t] = row[t] < c.n_rows;
        }
        for (int ks = ks0; ks < ks1; ks += POL_KU) {
            double a[POL_KU][POL_RT], b[POL_KU], m[POL_KU], dn[POL_KU];
            bool kin[POL_KU];
#pragma unroll
            for (int u = 0; u < POL_KU; u++) {  // the loads of POL_KU k-steps; a step beyond the run contributes 0 * 0
                const int k = uhc_pol_ab_k(lane, ks + u);
                kin[u] = ks + u < ks1 && k < d.K;
                b[u] = ks + u < ks1 ? wp[(size_t)(ks + u) * 64] : 0.0;
                m[u] = 0.0, dn[u] = 1.0;
                if (kin[u] && c.filter_on) m[u] = c.filt[k], dn[u] = c.filt[c.obs_dim + k];
#pragma unroll
                for (int t = 0; t < POL_RT; t++) a[u][t] = (kin[u] && live[t]) ? c.obs[row[t] * c.obs_stride + k] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < POL_KU; u++) {
                const int k = uhc_pol_ab_k(lane, ks + u);
#pragma unroll
                for (int t = 0; t < POL_RT; t++) {
                    if (kin[u] && live[t]) {
                        if (c.filter_on) a[u][t] = uhc_pol_filter(a[u][t], m[u], dn[u], c.demean, c.destd, c.clip);
                        if (writer) c.state_out[row[t] * c.obs_dim + k] = a[u][t];
                    }
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][t], b[u], acc[t], 0, 0, 0);
                }
            }
        }
    } else {
        const double* __restrict__ xp = c.x + d.in_off + lane;  // (lane l reads slot l of a k-step: uhc_pol_x_index)
        for (int ks = ks0; ks < ks1; ks += POL_KU) {
            double a[POL_KU][POL_RT], b[POL_KU];
#pragma unroll
            for (int u = 0; u < POL_KU; u++) {
                const bool in = ks + u < ks1;
                b[u] = in ? wp[(size_t)(ks + u) * 64] : 0.0;
#pragma unroll
                for (int t = 0; t < POL_RT; t++) a[u][t] = (in && rt0 + t < ntile) ? xp[((size_t)(rt0 + t) * ksteps + ks + u) * 64] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < POL_KU; u++)
#pragma unroll
                for (int t = 0; t < POL_RT; t++) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][t], b[u], acc[t], 0, 0, 0);
        }
    }

    // the four runs of K, added in wave order
#pragma unroll
    for (int t = 0; t < POL_RT; t++)
#pragma unroll
        for (int i = 0; i < 4; i++) part[wave][t][i][lane] = acc[t][i];
    __syncthreads();
    const int t = wave;  // this wave's row tile
    if (rt0 + t >= ntile) return;
    // bias, activation, store: register i of lane l is (row (l >> 4) + 4 i, column l & 15) of the tile
    const int col = 16 * ct + uhc_pol_cd_col(lane);
    const double bias = c.b[d.b_off + col];  // (padded to 16: in bounds)
    const int npad4 = uhc_pol_pad4(d.N);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double s = part[0][t][i][lane];
#pragma unroll
        for (int w = 1; w < POL_WAVES; w++) s += part[w][t][i][lane];
        const int r = 16 * (rt0 + t) + uhc_pol_cd_row(lane, i);
        const double v = uhc_pol_act(d.act, s + bias);
        if (d.final) {
            if (r < c.n_rows && col < d.N) c.fin[d.out_off + (size_t)r * d.N + col] = v;
        } else if (col < npad4) {  // the padding columns are exact zeros, whatever the activation makes of 0
            c.x[d.out_off + uhc_pol_x_index(r, col, npad4)] = col < d.N ? v : 0.0;
        }
    }
}

// ------------------------------------------------------------------ MCP: softmax of the composer, weighted sum of the primitives
// one thread per (row, action component); products and sums rounded separately, p ascending
__global__ void __launch_bounds__(256) uhc_policy_combine_kernel(const double* __restrict__ fin, int n_rows, int max_rows, int P, int act_dim,
                                                                 double* __restrict__ mean, double* __restrict__ weight_out) {
#pragma clang fp contract(off)
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)n_rows * act_dim) return;
    const int r = (int)(idx / act_dim), j = (int)(idx % act_dim);
    const double* cw = fin + (size_t)P * max_rows * act_dim + (size_t)r * P;
    double mx = cw[0];
    for (int p = 1; p < P; p++) mx = cw[p] > mx ? cw[p] : mx;
    double s = 0.0;
    for (int p = 0; p < P; p++) s += exp(cw[p] - mx);
    double a = 0.0;
    for (int p = 0; p < P; p++) {
        const double w = exp(cw[p] - mx) / s;
        if (j == 0 && weight_out) weight_out[(size_t)r * P + p] = w;
        a += w * fin[((size_t)p * max_rows + r) * act_dim + j];
    }
    mean[idx] = a;
}

// ------------------------------------------------------------------ host
static void pol_free(UhcPolicy* p) {
    if (!p) return;
    void* all[] = {p->d_raw, p->d_w, p->d_b, p->d_x, p->d_final, p->d_filt, p->d_filt_in, p->d_desc};
    for (void* q : all)
        if (q) (void)hipFree(q);
    delete p;
}

// raw weights (device or host arrays, flat layer order) -> d_raw -> packed, on stream st
static int pol_set_params(hipStream_t st, UhcPolicy* p, const double* const* w, const double* const* b, bool on_device) {
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    for (int net = 0; net < p->n_nets; net++)
        for (int l = 0; l < p->n_layers[net]; l++) {
            const int f = p->first[net] + l, N = p->widths[f], K = p->in_dim(net, l);
            HIP_OK(hipMemcpyAsync(p->d_raw + p->raw_w[f], w[f], sizeof(double) * N * K, kind, st));
            HIP_OK(hipMemcpyAsync(p->d_raw + p->raw_b[f], b[f], sizeof(double) * N, kind, st));
            const PolDesc& d = p->desc[(size_t)l * p->n_nets + net];
            const long long total = (long long)uhc_pol_w_doubles(N, K) + uhc_pol_pad16(N);
            hipLaunchKernelGGL(uhc_policy_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, p->d_raw + p->raw_w[f], p->d_raw + p->raw_b[f], N, K,
                               p->d_w + d.w_off, p->d_b + d.b_off);
            HIP_OK(hipGetLastError());
        }
    return 0;
}

extern "C" int32_t uhc_policy_create(int32_t kind, int32_t obs_dim, int32_t act_dim, int32_t max_rows, int32_t n_nets, const int32_t* h_n_layers,
                                     const int32_t* h_widths, const int32_t* h_acts, const double* const* h_w, const double* const* h_b, UhcPolicy** out) {
    // every check comes before the first HIP call
    const char* fn = "uhc_policy_create";
    REFUSE(fn, !out || !h_n_layers || !h_widths || !h_acts || !h_w || !h_b, "NULL argument");
    *out = nullptr;
    REFUSE(fn, kind != UHC_POLICY_GAUSSIAN && kind != UHC_POLICY_MCP, "unknown kind");
    REFUSE(fn, obs_dim <= 0 || act_dim <= 0 || max_rows <= 0 || n_nets <= 0, "non-positive dimension");
    REFUSE(fn, obs_dim > POL_MAX_DIM || act_dim > POL_MAX_DIM || max_rows > POL_MAX_DIM || n_nets > POL_MAX_NETS, "dimension too large");
    REFUSE(fn, kind == UHC_POLICY_GAUSSIAN && n_nets != 1, "a Gaussian policy is one net");
    REFUSE(fn, kind == UHC_POLICY_MCP && n_nets < 2, "an MCP policy is at least one primitive and the composer");
    UhcPolicy* p = new UhcPolicy;
    struct Guard {  // (REFUSE returns: the handle goes with it)
        UhcPolicy*& p;
        ~Guard() { pol_free(p); }
    } guard{p};
    p->kind = kind, p->obs_dim = obs_dim, p->act_dim = act_dim, p->max_rows = max_rows, p->n_nets = n_nets;
    p->P = kind == UHC_POLICY_MCP ? n_nets - 1 : 0;
    int flat = 0;
    for (int net = 0; net < n_nets; net++) {
        REFUSE(fn, h_n_layers[net] <= 0, "non-positive dimension");
        REFUSE(fn, h_n_layers[net] > POL_MAX_LAYERS, "dimension too large");
        p->n_layers.push_back(h_n_layers[net]);
        p->first.push_back(flat);
        for (int l = 0; l < h_n_layers[net]; l++, flat++) {
            REFUSE(fn, h_widths[flat] <= 0, "non-positive dimension");
            REFUSE(fn, h_widths[flat] > POL_MAX_DIM, "dimension too large");
            REFUSE(fn, h_acts[flat] < 0 || h_acts[flat] >= UHC_POL_N_ACT, "unknown activation");
            p->widths.push_back(h_widths[flat]);
            p->acts.push_back(h_acts[flat]);
        }
        p->depth = h_n_layers[net] > p->depth ? h_n_layers[net] : p->depth;
    }
    const int n_out = kind == UHC_POLICY_MCP ? p->P : 1;  // the nets whose result is an action mean
    for (int net = 0; net < n_out; net++) {
        bool same = p->n_layers[net] == p->n_layers[0];
        for (int l = 0; same && l < p->n_layers[0]; l++) same = p->widths[p->first[net] + l] == p->widths[l] && p->acts[p->first[net] + l] == p->acts[l];
        REFUSE(fn, !same, "primitives of unequal shape");
        REFUSE(fn, p->widths[p->first[net] + p->n_layers[net] - 1] != act_dim, "a net's last width is not act_dim");
    }
    if (kind == UHC_POLICY_MCP) REFUSE(fn, p->widths[flat - 1] != p->P, "the composer's last width is not the number of primitives");
    for (int net = 0; net < n_nets; net++)
        for (int l = 0; l < p->n_layers[net]; l++) {
            const int f = p->first[net] + l;
            REFUSE(fn, !h_w[f] || !h_b[f], "NULL weight or bias array");
            REFUSE(fn, !uhc_all_finite(h_w[f], (size_t)p->widths[f] * p->in_dim(net, l)) || !uhc_all_finite(h_b[f], (size_t)p->widths[f]), "non-finite weight");
        }
    // the layout: raw, packed weights, biases, activations between the layers, the nets' results (MCP)
    size_t nw = 0, nb = 0, nx = 0;
    p->raw_w.resize(flat), p->raw_b.resize(flat);
    p->desc.assign((size_t)p->depth * n_nets, PolDesc{0, 0, 0, 0, 0, 0, 0, 0});
    for (int net = 0; net < n_nets; net++) {
        long long prev_out = 0;
        for (int l = 0; l < p->n_layers[net]; l++) {
            const int f = p->first[net] + l, N = p->widths[f], K = p->in_dim(net, l);
            p->raw_w[f] = p->raw_total, p->raw_total += (size_t)N * K;
            p->raw_b[f] = p->raw_total, p->raw_total += (size_t)N;
            PolDesc& d = p->desc[(size_t)l * n_nets + net];
            d.K = K, d.N = N, d.act = p->acts[f], d.final = l == p->n_layers[net] - 1;
            d.w_off = (long long)nw, nw += uhc_pol_w_doubles(N, K);
            d.b_off = (long long)nb, nb += (size_t)uhc_pol_pad16(N);
            d.in_off = prev_out;
            if (d.final) {
                // Gaussian: the caller's d_mean.  MCP: [P][max_rows][act_dim], then the composer's [max_rows][P]
                d.out_off = kind == UHC_POLICY_MCP ? (long long)((size_t)(net < p->P ? net : p->P) * max_rows * act_dim) : 0;
            } else {
                d.out_off = prev_out = (long long)nx, nx += uhc_pol_x_doubles(max_rows, N);
            }
        }
    }
    p->n_packed = nw + nb;
    HIP_OK(hipMalloc((void**)&p->d_raw, sizeof(double) * p->raw_total));
    HIP_OK(hipMalloc((void**)&p->d_w, sizeof(double) * nw));
    HIP_OK(hipMalloc((void**)&p->d_b, sizeof(double) * nb));
    HIP_OK(hipMalloc((void**)&p->d_x, sizeof(double) * (nx > 0 ? nx : 1)));
    HIP_OK(hipMemset(p->d_x, 0, sizeof(double) * (nx > 0 ? nx : 1)));
    if (kind == UHC_POLICY_MCP) {
        const size_t nf = (size_t)p->P * max_rows * act_dim + (size_t)max_rows * p->P;
        HIP_OK(hipMalloc((void**)&p->d_final, sizeof(double) * nf));
        HIP_OK(hipMemset(p->d_final, 0, sizeof(double) * nf));
    }
    HIP_OK(hipMalloc((void**)&p->d_filt, sizeof(double) * 2 * obs_dim));
    HIP_OK(hipMalloc((void**)&p->d_filt_in, sizeof(double) * (1 + 2 * (size_t)obs_dim)));
    HIP_OK(uhc_upload(&p->d_desc, p->desc.data(), p->desc.size()));
    if (pol_set_params(nullptr, p, h_w, h_b, false)) return 1;
    HIP_OK(hipStreamSynchronize(nullptr));
    *out = p;
    p = nullptr;  // (the guard lets it live)
    return 0;
}

extern "C" void uhc_policy_free(UhcPolicy* p) { pol_free(p); }

extern "C" int32_t uhc_policy_dims(const UhcPolicy* p, int32_t* kind, int32_t* obs_dim, int32_t* act_dim, int32_t* max_rows, int32_t* n_primitives,
                                   int64_t* packed_bytes) {
    REFUSE("uhc_policy_dims", !p, "NULL policy");
    if (kind) *kind = p->kind;
    if (obs_dim) *obs_dim = p->obs_dim;
    if (act_dim) *act_dim = p->act_dim;
    if (max_rows) *max_rows = p->max_rows;
    if (n_primitives) *n_primitives = p->P;
    if (packed_bytes) *packed_bytes = (int64_t)(sizeof(double) * p->n_packed);
    return 0;
}

extern "C" int32_t uhc_policy_set_filter(UhcPolicy* p, double n, const double* h_mean, const double* h_S, int32_t demean, int32_t destd, double clip) {
    const char* fn = "uhc_policy_set_filter";
    REFUSE(fn, !p, "NULL policy");
    if (!h_mean && !h_S) {  // no filter: observations go in as they are
        p->has_filter = p->demean = p->destd = 0;  // (the switches too: uhc_policy_save writes them)
        p->clip = p->filt_n = 0.0;
        return 0;
    }
    REFUSE(fn, !h_mean || !h_S, "mean and S come together");
    REFUSE(fn, !(n >= 0.0) || !std::isfinite(n) || !(clip >= 0.0) || !std::isfinite(clip), "n and clip are finite and not negative");
    REFUSE(fn, !uhc_all_finite(h_mean, p->obs_dim) || !uhc_all_finite(h_S, p->obs_dim), "non-finite statistics");
    std::vector<double> in(1 + 2 * (size_t)p->obs_dim);
    in[0] = n;
    memcpy(&in[1], h_mean, sizeof(double) * p->obs_dim);
    memcpy(&in[1 + p->obs_dim], h_S, sizeof(double) * p->obs_dim);
    HIP_OK(hipDeviceSynchronize());  // (a call still running reads the old table)
    HIP_OK(hipMemcpy(p->d_filt_in, in.data(), sizeof(double) * in.size(), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(uhc_policy_filter_kernel, dim3((unsigned)((p->obs_dim + 255) / 256)), dim3(256), 0, nullptr, p->d_filt_in, p->obs_dim, p->d_filt);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(nullptr));
    p->has_filter = 1, p->demean = demean != 0, p->destd = destd != 0, p->clip = clip, p->filt_n = n;
    p->filt_mean.assign(h_mean, h_mean + p->obs_dim);
    p->filt_S.assign(h_S, h_S + p->obs_dim);
    return 0;
}

extern "C" int32_t uhc_policy_set_params(void* stream, UhcPolicy* p, const double* const* w, const double* const* b, int32_t on_device) {
    const char* fn = "uhc_policy_set_params";
    REFUSE(fn, !p || !w || !b, "NULL argument");
    const size_t flat = p->widths.size();
    for (size_t f = 0; f < flat; f++) REFUSE(fn, !w[f] || !b[f], "NULL weight or bias array");
    if (!on_device)
        for (int net = 0; net < p->n_nets; net++)
            for (int l = 0; l < p->n_layers[net]; l++) {
                const int f = p->first[net] + l;
                REFUSE(fn, !uhc_all_finite(w[f], (size_t)p->widths[f] * p->in_dim(net, l)) || !uhc_all_finite(b[f], (size_t)p->widths[f]), "non-finite weight");
            }
    if (pol_set_params((hipStream_t)stream, p, w, b, on_device != 0)) return 1;
    if (!on_device) HIP_OK(hipStreamSynchronize((hipStream_t)stream));  // host arrays are the caller's again when the call returns
    return 0;
}

extern "C" int32_t uhc_policy_act(void* stream, UhcPolicy* p, int32_t n_rows, const double* d_obs, int64_t obs_stride, double* d_state_out, double* d_mean,
                                  double* d_weight_out) {
    const char* fn = "uhc_policy_act";
    REFUSE(fn, !p, "NULL policy");
    REFUSE(fn, n_rows < 0, "negative n_rows");
    if (n_rows == 0) return 0;
    REFUSE(fn, n_rows > p->max_rows, "n_rows = " + std::to_string(n_rows) + " is above the handle's max_rows = " + std::to_string(p->max_rows));
    REFUSE(fn, obs_stride < p->obs_dim, "obs_stride = " + std::to_string((long long)obs_stride) + " is below obs_dim = " + std::to_string(p->obs_dim));
    REFUSE(fn, !d_obs || !d_mean, "NULL d_obs or d_mean");
    REFUSE(fn, d_weight_out && p->kind != UHC_POLICY_MCP, "d_weight_out: a Gaussian policy has no composer");
    hipStream_t st = (hipStream_t)stream;
    PolCall c;
    c.w = p->d_w, c.b = p->d_b, c.x = p->d_x;
    c.fin = p->kind == UHC_POLICY_MCP ? p->d_final : d_mean;
    c.obs = d_obs, c.obs_stride = obs_stride, c.state_out = d_state_out, c.filt = p->d_filt;
    c.n_rows = n_rows, c.obs_dim = p->obs_dim, c.filter_on = p->has_filter, c.demean = p->demean, c.destd = p->destd, c.clip = p->clip;
    const unsigned gy = (unsigned)(((n_rows + 15) / 16 + POL_RT - 1) / POL_RT);
    for (int l = 0; l < p->depth; l++) {
        int nmax = 0;
        for (int net = 0; net < p->n_nets; net++) nmax = p->desc[(size_t)l * p->n_nets + net].N > nmax ? p->desc[(size_t)l * p->n_nets + net].N : nmax;
        const dim3 grid((unsigned)(uhc_pol_pad16(nmax) / 16), gy, (unsigned)p->n_nets);
        const PolDesc* dl = p->d_desc + (size_t)l * p->n_nets;
        if (l == 0)
            hipLaunchKernelGGL(uhc_policy_layer_kernel<true>, grid, dim3(64 * POL_WAVES), 0, st, c, dl);
        else
            hipLaunchKernelGGL(uhc_policy_layer_kernel<false>, grid, dim3(64 * POL_WAVES), 0, st, c, dl);
        HIP_OK(hipGetLastError());
    }
    if (p->kind == UHC_POLICY_MCP) {
        const long long total = (long long)n_rows * p->act_dim;
        hipLaunchKernelGGL(uhc_policy_combine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, p->d_final, n_rows, p->max_rows, p->P, p->act_dim,
                           d_mean, d_weight_out);
        HIP_OK(hipGetLastError());
    }
    return 0;
}

// ------------------------------------------------------------------ the file: what a C program deploys
//   uint64 magic "UHCPOLCY", int32 version (1), kind, obs_dim, act_dim, n_nets, n_layers[n_nets], widths[flat], acts[flat],
//   int32 has_filter, demean, destd, 0, double clip, n, mean[obs_dim], S[obs_dim] (zeros without a filter),
//   double raw[raw_total]: per net, per layer, W [out][in] then b [out]
static const uint64_t POL_MAGIC = 0x59434c4f50434855ULL;  // "UHCPOLCY" as it lies in the file
#define POL_FILE_VERSION 1

extern "C" int32_t uhc_policy_save(const UhcPolicy* p, const char* path) {
    const char* fn = "uhc_policy_save";
    REFUSE(fn, !p || !path, "NULL argument");
    std::vector<double> raw(p->raw_total);
    HIP_OK(hipDeviceSynchronize());  // (a uhc_policy_set_params still in flight on some stream)
    HIP_OK(hipMemcpy(raw.data(), p->d_raw, sizeof(double) * p->raw_total, hipMemcpyDeviceToHost));
    std::vector<int32_t> head = {POL_FILE_VERSION, p->kind, p->obs_dim, p->act_dim, p->n_nets};
    head.insert(head.end(), p->n_layers.begin(), p->n_layers.end());
    head.insert(head.end(), p->widths.begin(), p->widths.end());
    head.insert(head.end(), p->acts.begin(), p->acts.end());
    const int32_t fl[4] = {p->has_filter, p->demean, p->destd, 0};
    head.insert(head.end(), fl, fl + 4);
    std::vector<double> filt(2 + 2 * (size_t)p->obs_dim, 0.0);
    if (p->has_filter) {
        filt[0] = p->clip, filt[1] = p->filt_n;
        memcpy(&filt[2], p->filt_mean.data(), sizeof(double) * p->obs_dim);
        memcpy(&filt[2 + p->obs_dim], p->filt_S.data(), sizeof(double) * p->obs_dim);
    }
    FILE* f = fopen(path, "wb");
    REFUSE(fn, !f, std::string("cannot open ") + path);
    bool ok = fwrite(&POL_MAGIC, sizeof(POL_MAGIC), 1, f) == 1 && fwrite(head.data(), sizeof(int32_t), head.size(), f) == head.size() &&
              fwrite(filt.data(), sizeof(double), filt.size(), f) == filt.size() && fwrite(raw.data(), sizeof(double), raw.size(), f) == raw.size();
    ok = (fclose(f) == 0) && ok;
    REFUSE(fn, !ok, std::string("cannot write ") + path);
    return 0;
}

extern "C" int32_t uhc_policy_load(const char* path, int32_t max_rows, UhcPolicy** out) {
    const char* fn = "uhc_policy_load";
    REFUSE(fn, !path || !out, "NULL argument");
    *out = nullptr;
    FILE* f = fopen(path, "rb");
    REFUSE(fn, !f, std::string("cannot open ") + path);
    struct Closer {
        FILE* f;
        ~Closer() { fclose(f); }
    } closer{f};
    // Nothing is sized from the header before the file is known to hold it: a malformed file is refused, it cannot ask for memory the host does not have
    REFUSE(fn, fseek(f, 0, SEEK_END) != 0, "cannot read the file");
    const long fsize = ftell(f);
    REFUSE(fn, fsize < 0 || fseek(f, 0, SEEK_SET) != 0, "cannot read the file");
    auto left = [&]() -> size_t { const long at = ftell(f); return at < 0 || at > fsize ? 0 : (size_t)(fsize - at); };
    uint64_t magic = 0;
    int32_t h[5] = {0, 0, 0, 0, 0};
    REFUSE(fn, fread(&magic, sizeof(magic), 1, f) != 1 || magic != POL_MAGIC, "not a policy file");
    REFUSE(fn, fread(h, sizeof(int32_t), 5, f) != 5, "truncated file");
    REFUSE(fn, h[0] != POL_FILE_VERSION, "unknown file version");
    const int32_t kind = h[1], obs_dim = h[2], act_dim = h[3], n_nets = h[4];
    REFUSE(fn, obs_dim <= 0 || obs_dim > POL_MAX_DIM || act_dim <= 0 || act_dim > POL_MAX_DIM || n_nets <= 0 || n_nets > POL_MAX_NETS, "bad header");
    std::vector<int32_t> n_layers(n_nets);
    REFUSE(fn, fread(n_layers.data(), sizeof(int32_t), n_nets, f) != (size_t)n_nets, "truncated file");
    size_t flat = 0;
    for (int32_t v : n_layers) {
        REFUSE(fn, v <= 0 || v > POL_MAX_LAYERS, "bad header");
        flat += (size_t)v;
    }
    std::vector<int32_t> widths(flat), acts(flat);
    int32_t fl[4];
    REFUSE(fn, fread(widths.data(), sizeof(int32_t), flat, f) != flat || fread(acts.data(), sizeof(int32_t), flat, f) != flat || fread(fl, sizeof(int32_t), 4, f) != 4,
           "truncated file");
    REFUSE(fn, left() / sizeof(double) < 2 + 2 * (size_t)obs_dim, "truncated file");
    std::vector<double> filt(2 + 2 * (size_t)obs_dim);
    REFUSE(fn, fread(filt.data(), sizeof(double), filt.size(), f) != filt.size(), "truncated file");
    size_t total = 0;
    std::vector<size_t> w_at(flat), b_at(flat);
    for (size_t net = 0, i = 0; net < (size_t)n_nets; net++)
        for (int l = 0; l < n_layers[net]; l++, i++) {
            REFUSE(fn, widths[i] <= 0 || widths[i] > POL_MAX_DIM, "bad header");
            const size_t K = l == 0 ? (size_t)obs_dim : (size_t)widths[i - 1];
            w_at[i] = total, total += (size_t)widths[i] * K;
            b_at[i] = total, total += (size_t)widths[i];
        }
    REFUSE(fn, left() / sizeof(double) < total, "truncated file");
    std::vector<double> raw(total);
    REFUSE(fn, fread(raw.data(), sizeof(double), total, f) != total, "truncated file");
    std::vector<const double*> w(flat), b(flat);
    for (size_t i = 0; i < flat; i++) w[i] = raw.data() + w_at[i], b[i] = raw.data() + b_at[i];
    UhcPolicy* p = nullptr;
    if (uhc_policy_create(kind, obs_dim, act_dim, max_rows, n_nets, n_layers.data(), widths.data(), acts.data(), w.data(), b.data(), &p)) return 1;
    if (fl[0] && uhc_policy_set_filter(p, filt[1], &filt[2], &filt[2 + obs_dim], fl[1], fl[2], filt[0])) {
        pol_free(p);
        return 1;
    }
    *out = p;
    return 0;
}
