// Beam search step of the graphed decode (HF GenerationMixin._beam_search, transformers 5.15; llamole_amd/llm_beam.py is the torch
// statement of the same step and documents the state layout) and the in-place KV-cache reorder by the beams' parents.
//   beam_rows_kernel   : one workgroup per row (beam) -- f32 log-sum-exp, then the row's candidates: greedy = its K largest logits
//                        (16-bit radix select on order-preserving bf16 keys; ties at the K-th key by lower token index); beam sample =
//                        the top-k' survivors (k' = max(top_k, n_eos + 1), ties kept), HF's TopP with min_tokens_to_keep on their
//                        sorted list, then Gumbel keys acc - log(E) with E ~ Exp(1) from Philox keyed by (seed, step, row, token);
//                        the K best by key go to the state's candidate slots.  Bound that depends on the data: a row whose top-k'
//                        threshold value is shared by more tokens than fit the 1024-entry list keeps the lowest-indexed of them
//                        (HF keeps them all); with top_k <= 512 that takes over 500 equal bf16 logits at the threshold.
//   beam_item_kernel   : one workgroup per batch item -- the global stop of the last step, the merge of the item's nb*K candidates to
//                        K, EOS / max-length hits, running beams, finished hypotheses with the length penalty, the early-stop
//                        heuristic; writes the next input tokens, the parents and the position counters.
//   beam_kv_reorder_kernel : one workgroup per tile (tensor, item, kv head, slot chunk) owns all nb beams of the tile: every thread
//                        loads what it will store, a barrier, then the stores -- in place, no scratch.
// Every score is f32 in HF's order of operations with its -1e9 constants; ties: a higher score first, then the lower flat index.
#include "common.h"

namespace ll {
namespace {

constexpr int ROW_THREADS = 512;
constexpr int ROW_CAP = 1024;        // survivor list of one row (beam sample: k' <= 512 plus ties)
constexpr int ITEM_THREADS = 256;
constexpr int ITEM_CAP = 4096;       // nb * K of one item
constexpr float NEG = -1.0e9f;

// state segments (llm_beam.py _SEGMENTS): int32 / f32 words, each padded to a multiple of 4
struct BeamState {
    float *run, *hyp;
    int *fin, *hyp_t, *hyp_beam, *hyp_tok, *flags, *par, *rtok, *rpar;
    uint32_t *cand;
};
__host__ __device__ inline int64_t pad4(int64_t n) { return (n + 3) / 4 * 4; }
__host__ __device__ inline int64_t state_words(int B, int nb, int K, int T) {
    const int64_t R = (int64_t)B * nb;
    return 6 * pad4(R) + pad4(8 * (int64_t)B) + pad4(R) + 2 * pad4(R * T) + pad4(R * K * 3);
}
__host__ __device__ inline BeamState state_of(void *base, int B, int nb, int K, int T) {
    const int64_t R = (int64_t)B * nb;
    int *w = (int *)base;
    BeamState s;
    s.run = (float *)w; w += pad4(R);
    s.hyp = (float *)w; w += pad4(R);
    s.fin = w; w += pad4(R);
    s.hyp_t = w; w += pad4(R);
    s.hyp_beam = w; w += pad4(R);
    s.hyp_tok = w; w += pad4(R);
    s.flags = w; w += pad4(8 * (int64_t)B);
    s.par = w; w += pad4(R);
    s.rtok = w; w += pad4(R * T);
    s.rpar = w; w += pad4(R * T);
    s.cand = (uint32_t *)w;
    (void)K;
    return s;
}

__device__ __forceinline__ uint32_t bkey(uint32_t x) { return (x & 0x8000u) ? (~x & 0xFFFFu) : (x | 0x8000u); }   // bf16 bits -> order
__device__ __forceinline__ uint32_t bkey_inv(uint32_t k) { return (k & 0x8000u) ? (k ^ 0x8000u) : (~k & 0xFFFFu); }
__device__ __forceinline__ uint32_t fkey(float f) {                                                                // f32 -> order
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct RowArgs {
    const bf16_t *logits;
    int64_t ld;
    int B, nb, V, K, T;
    void *state;
    int do_sample, top_k, min_keep;
    float inv_temp, top_p;
    const int64_t *seed;
};

struct RowLds {
    uint32_t hist[256];
    unsigned long long list[ROW_CAP];     // (key << 32) | ~token: descending = larger key, then lower token
    float tail[ROW_CAP];
    float acc[ROW_CAP];
    float red[ROW_THREADS / 64 * 2];
    uint32_t n, sel, need, above;
};

// block-wide: the bin b (scanning from 255 down) where the running count first reaches `want`; returns the count above it in *above
__device__ uint32_t hist_pick(RowLds &L, uint32_t want, uint32_t *above) {
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0, b = 255;
        for (;; --b) {
            if (c + L.hist[b] >= want || b == 0) break;
            c += L.hist[b];
        }
        L.sel = b;
        L.above = c;
    }
    __syncthreads();
    *above = L.above;
    return L.sel;
}

// bitonic sort of L.list[0, n2) descending (n2 a power of two); `pay` (optional) moves along
__device__ void sort_desc(unsigned long long *a, float *pay, int n2, int nthreads) {
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int i = threadIdx.x; i < n2; i += nthreads) {
                const int l = i ^ j;
                if (l > i) {
                    const bool desc = (i & k) == 0;
                    const unsigned long long x = a[i], y = a[l];
                    if (desc ? (x < y) : (x > y)) {
                        a[i] = y;
                        a[l] = x;
                        if (pay) { const float t = pay[i]; pay[i] = pay[l]; pay[l] = t; }
                    }
                }
            }
        }
    __syncthreads();
}

__device__ __forceinline__ float block_sum(float v, float *red) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    float s = 0.f;
    for (int i = 0; i < nw; ++i) s += red[i];
    return s;
}
__device__ __forceinline__ float block_max(float v, float *red) {
    v = wave_max(v);
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    float s = -INFINITY;
    for (int i = 0; i < nw; ++i) s = fmaxf(s, red[i]);
    return s;
}

__global__ __launch_bounds__(ROW_THREADS) void beam_rows_kernel(RowArgs a) {
    __shared__ RowLds L;
    const int r = blockIdx.x, tid = threadIdx.x;
    const int item = r / a.nb;
    BeamState S = state_of(a.state, a.B, a.nb, a.K, a.T);
    const uint4 *row = (const uint4 *)(a.logits + (int64_t)r * a.ld);
    const int nvec = a.V / 8;
    // ---- pass 1: row maximum and high-byte histogram of the keys
    for (int i = tid; i < 256; i += ROW_THREADS) L.hist[i] = 0;
    __syncthreads();
    float m = -INFINITY;
    for (int v = tid; v < nvec; v += ROW_THREADS) {
        const uint4 q = row[v];
        const uint32_t w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int h = 0; h < 8; ++h) {
            const uint32_t x = (w4[h >> 1] >> ((h & 1) * 16)) & 0xFFFFu;
            m = fmaxf(m, __uint_as_float(x << 16));
            atomicAdd(&L.hist[bkey(x) >> 8], 1u);
        }
    }
    m = block_max(m, L.red);
    // ---- pass 2: sum of exp(x - m) (log_softmax: (x - m) - log(sum))
    float s = 0.f;
    for (int v = tid; v < nvec; v += ROW_THREADS) {
        const uint4 q = row[v];
        const uint32_t w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int h = 0; h < 8; ++h) s += expf(__uint_as_float(((w4[h >> 1] >> ((h & 1) * 16)) & 0xFFFFu) << 16) - m);
    }
    const float logsum = logf(block_sum(s, L.red + ROW_THREADS / 64));
    // ---- the k-th largest key: kc = K (greedy) or k' (sample)
    const int kc = a.do_sample ? min(max(a.top_k, a.min_keep), a.V) : a.K;
    uint32_t above_hi;
    const uint32_t hb = hist_pick(L, (uint32_t)kc, &above_hi);
    for (int i = tid; i < 256; i += ROW_THREADS) L.hist[i] = 0;
    __syncthreads();
    for (int v = tid; v < nvec; v += ROW_THREADS) {
        const uint4 q = row[v];
        const uint32_t w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int h = 0; h < 8; ++h) {
            const uint32_t k = bkey((w4[h >> 1] >> ((h & 1) * 16)) & 0xFFFFu);
            if ((k >> 8) == hb) atomicAdd(&L.hist[k & 255u], 1u);
        }
    }
    uint32_t above_lo;
    const uint32_t lb = hist_pick(L, (uint32_t)kc - above_hi, &above_lo);
    const uint32_t kth = (hb << 8) | lb;
    const uint32_t above = above_hi + above_lo;          // keys > kth
    const uint32_t ties = L.hist[lb];
    // greedy: exactly K = above + the (K - above) lowest-indexed ties; sample: every tie (up to the list's room)
    const uint32_t need = a.do_sample ? min(ties, (uint32_t)ROW_CAP - above) : (uint32_t)kc - above;
    // the lowest `need` tie indices: the largest index taken (a radix select over the token index when not all ties fit)
    uint32_t idx_cut = 0xFFFFFFFFu;
    if (need < ties) {
        uint32_t want = need, prefix = 0;
        for (int shift = 16; shift >= 0; shift -= 8) {
            __syncthreads();
            for (int i = tid; i < 256; i += ROW_THREADS) L.hist[i] = 0;
            __syncthreads();
            for (int v = tid; v < nvec; v += ROW_THREADS) {
                const uint4 q = row[v];
                const uint32_t w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int h = 0; h < 8; ++h) {
                    const uint32_t k = bkey((w4[h >> 1] >> ((h & 1) * 16)) & 0xFFFFu);
                    const uint32_t t = (uint32_t)(v * 8 + h);
                    if (k == kth && (shift == 16 || (t >> (shift + 8)) == prefix)) atomicAdd(&L.hist[(t >> shift) & 255u], 1u);
                }
            }
            __syncthreads();
            if (tid == 0) {          // smallest bin where the ascending count reaches want
                uint32_t c = 0, b = 0;
                for (; b < 255; ++b) {
                    if (c + L.hist[b] >= want) break;
                    c += L.hist[b];
                }
                L.sel = b;
                L.need = want - c;
            }
            __syncthreads();
            prefix = (shift == 16 ? 0u : prefix << 8) | L.sel;
            want = L.need;
        }
        idx_cut = prefix;
    }
    // ---- collect: keys > kth, and ties with index <= idx_cut
    if (tid == 0) L.n = 0;
    __syncthreads();
    for (int v = tid; v < nvec; v += ROW_THREADS) {
        const uint4 q = row[v];
        const uint32_t w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int h = 0; h < 8; ++h) {
            const uint32_t k = bkey((w4[h >> 1] >> ((h & 1) * 16)) & 0xFFFFu);
            const uint32_t t = (uint32_t)(v * 8 + h);
            if (k > kth || (k == kth && t <= idx_cut)) {
                const uint32_t slot = atomicAdd(&L.n, 1u);
                if (slot < ROW_CAP) L.list[slot] = ((unsigned long long)k << 32) | (0xFFFFFFFFu - t);
            }
        }
    }
    __syncthreads();
    const int n = (int)min(L.n, (uint32_t)ROW_CAP);
    const float run = S.run[r];
    uint32_t *cand = S.cand + (int64_t)r * a.K * 3;
    auto val_of = [&](unsigned long long e) { return __uint_as_float(bkey_inv((uint32_t)(e >> 32)) << 16); };
    if (!a.do_sample) {
        // exactly K entries: acc = log-prob + running score
        for (int i = tid; i < a.K; i += ROW_THREADS) {
            const unsigned long long e = L.list[i];
            const uint32_t t = 0xFFFFFFFFu - (uint32_t)e;
            const float acc = ((val_of(e) - m) - logsum) + run;
            cand[3 * i] = fkey(acc);
            cand[3 * i + 1] = __float_as_uint(acc);
            cand[3 * i + 2] = (uint32_t)((r % a.nb) * a.V) + t;
        }
        return;
    }
    // ---- beam sample: HF TopP (min_tokens_to_keep) on the survivors, in descending order.  Equal values: the higher token index first,
    // i.e. HF's ascending sort taken stably, so that at the nucleus boundary the lower-indexed of equal tokens is removed first
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    for (int i = tid; i < n2; i += ROW_THREADS)
        L.list[i] = i < n ? ((L.list[i] & 0xFFFFFFFF00000000ull) | (0xFFFFFFFFu - (uint32_t)L.list[i])) : 0ull;
    sort_desc(L.list, nullptr, n2, ROW_THREADS);
    const float s0 = ((val_of(L.list[0]) - m) - logsum) * a.inv_temp;
    float z = 0.f;
    for (int i = tid; i < n; i += ROW_THREADS) {
        const float si = ((val_of(L.list[i]) - m) - logsum) * a.inv_temp;
        L.acc[i] = si;
        L.tail[i] = expf(si - s0);
        z += L.tail[i];
    }
    z = block_sum(z, L.red);
    for (int i = tid; i < n2; i += ROW_THREADS) L.tail[i] = i < n ? L.tail[i] / z : 0.f;
    // suffix sums: tail[i] = sum of p[j], j >= i (HF's ascending cumulative sum at that token)
    for (int off = 1; off < n2; off <<= 1) {
        __syncthreads();
        float add[ROW_CAP / ROW_THREADS];
        int c = 0;
        for (int i = tid; i < n2; i += ROW_THREADS) add[c++] = i + off < n2 ? L.tail[i + off] : 0.f;
        __syncthreads();
        c = 0;
        for (int i = tid; i < n2; i += ROW_THREADS) L.tail[i] += add[c++];
    }
    __syncthreads();
    const float cut = (float)(1.0 - (double)a.top_p);
    const int64_t sd = *a.seed;
    const int step = S.flags[8 * item + 3];
    for (int i = tid; i < n2; i += ROW_THREADS) {
        float key = -INFINITY, acc = -INFINITY;
        if (i < n) {
            const bool removed = a.top_p < 1.f && L.tail[i] <= cut && i >= a.min_keep;
            if (!removed) {
                const uint32_t t = (uint32_t)L.list[i];
                acc = L.acc[i] + run;
                const uint4 rnd = philox4x32(make_uint4(t, (uint32_t)r, (uint32_t)step, 0xBEA5u), make_uint2((uint32_t)sd, (uint32_t)(sd >> 32)));
                key = acc - logf(exp1_from_bits(rnd.x));
            }
        }
        L.acc[i] = acc;
        const uint32_t t = i < n ? (uint32_t)L.list[i] : 0u;
        L.list[i] = i < n ? (((unsigned long long)fkey(key) << 32) | (0xFFFFFFFFu - t)) : 0ull;
    }
    sort_desc(L.list, L.acc, n2, ROW_THREADS);
    for (int i = tid; i < a.K; i += ROW_THREADS) {
        if (i < n) {
            const unsigned long long e = L.list[i];
            cand[3 * i] = (uint32_t)(e >> 32);
            cand[3 * i + 1] = __float_as_uint(L.acc[i]);
            cand[3 * i + 2] = (uint32_t)((r % a.nb) * a.V) + (0xFFFFFFFFu - (uint32_t)e);
        } else {                      // fewer survivors than K: a slot no selection reaches (key below every real one)
            cand[3 * i] = 0u;
            cand[3 * i + 1] = __float_as_uint(-INFINITY);
            cand[3 * i + 2] = (uint32_t)((r % a.nb) * a.V);
        }
    }
}
}  // namespace
}  // namespace ll

namespace ll {
namespace {

struct ItemArgs {
    int B, nb, V, K, T;
    void *state;
    const int64_t *eos;
    int n_eos, max_new;
    float length_penalty;
    int early_stopping;        // 0 False, 1 True, 2 "never"
    int64_t *tok, *posid, *pos;
    int advance;
};

struct ItemLds {
    unsigned long long key[ITEM_CAP];
    float acc[ITEM_CAP];
    float rs[512], fs[512];
    int beam[512], tok[512], hit[512];
    float ms[16 + 512];
    int sel_run[16], sel_hyp[16];
    float o_hyp[16];
    int o_fin[16], o_t[16], o_beam[16], o_tok[16];
    float n_hyp[16];
    int n_fin[16];
    int64_t eos[32];
    int stop, heur, full, allhit;
};

__global__ __launch_bounds__(ITEM_THREADS) void beam_item_kernel(ItemArgs a) {
    __shared__ ItemLds L;
    const int b = blockIdx.x, tid = threadIdx.x, nb = a.nb, K = a.K;
    BeamState S = state_of(a.state, a.B, nb, K, a.T);
    int *F = S.flags + 8 * b;
    const int t = F[3];
    const int cur = 4 * (t & 1), nxt = 4 - cur;     // the flags of the last step / of this one
    if (tid == 0) {
        int imp = 0, allfin = 1, allhit = 1;
        for (int i = 0; i < a.B; ++i) {
            const int *f = S.flags + 8 * i + cur;
            imp |= f[0];
            allfin &= f[1];
            allhit &= f[2];
        }
        L.stop = !(imp && !(allfin && a.early_stopping == 1) && !allhit);      // not _beam_search_has_unfinished_sequences
        L.heur = F[cur];
        int full = 1;
        for (int j = 0; j < nb; ++j) full &= S.fin[b * nb + j] != 0;
        L.full = full && a.early_stopping == 1;
        L.allhit = 1;
    }
    for (int i = tid; i < a.n_eos; i += ITEM_THREADS) L.eos[i] = a.eos[i];
    __syncthreads();
    if (L.stop) {                                    // a step after the global stop changes nothing
        if (tid < nb) S.par[b * nb + tid] = b * nb + tid;
        return;
    }
    // ---- the item's K best of nb * K row candidates
    const int N = nb * K;
    int n2 = 1;
    while (n2 < N) n2 <<= 1;
    for (int i = tid; i < n2; i += ITEM_THREADS) {
        if (i < N) {
            const uint32_t *c = S.cand + (int64_t)(b * nb) * K * 3 + 3 * i;
            L.key[i] = ((unsigned long long)c[0] << 32) | (0xFFFFFFFFu - c[2]);
            L.acc[i] = __uint_as_float(c[1]);
        } else {
            L.key[i] = 0ull;
            L.acc[i] = -INFINITY;
        }
    }
    sort_desc(L.key, L.acc, n2, ITEM_THREADS);
    const bool last = t + 1 >= a.max_new;
    for (int k = tid; k < K; k += ITEM_THREADS) {
        const uint32_t flat = 0xFFFFFFFFu - (uint32_t)L.key[k];
        const int bm = (int)(flat / (uint32_t)a.V), tk = (int)(flat % (uint32_t)a.V);
        int hit = last;
        for (int e = 0; e < a.n_eos; ++e) hit |= L.eos[e] == tk;
        const float acc = L.acc[k];
        L.beam[k] = bm;
        L.tok[k] = tk;
        L.hit[k] = hit;
        L.rs[k] = acc + (hit ? NEG : 0.f);
        if (!hit) atomicAnd(&L.allhit, 0);
    }
    if (tid < nb) {
        const int r = b * nb + tid;
        L.o_hyp[tid] = S.hyp[r];
        L.o_fin[tid] = S.fin[r];
        L.o_t[tid] = S.hyp_t[r];
        L.o_beam[tid] = S.hyp_beam[r];
        L.o_tok[tid] = S.hyp_tok[r];
    }
    __syncthreads();
    // finished candidates: acc / gen_len ** length_penalty (the power in double, the division as torch's reciprocal product), then -1e9 terms
    const float den = (float)pow((double)(t + 1), (double)a.length_penalty);
    const float inv_den = 1.0f / den;
    for (int k = tid; k < K; k += ITEM_THREADS) {
        const int did = L.hit[k] && k < nb;
        float s = L.acc[k] * inv_den;
        s = s + (L.full ? NEG : 0.f);
        s = s + (L.heur ? 0.f : NEG);
        s = s + (did ? 0.f : NEG);
        L.fs[k] = s;
        L.ms[nb + k] = s;
    }
    if (tid < nb) L.ms[tid] = L.o_hyp[tid];
    __syncthreads();
    // ranks: higher value first, then the lower index
    for (int k = tid; k < K; k += ITEM_THREADS) {
        const float v = L.rs[k];
        int rank = 0;
        for (int j = 0; j < K; ++j) rank += (L.rs[j] > v) || (L.rs[j] == v && j < k);
        if (rank < nb) L.sel_run[rank] = k;
    }
    for (int i = tid; i < nb + K; i += ITEM_THREADS) {
        const float v = L.ms[i];
        int rank = 0;
        for (int j = 0; j < nb + K; ++j) rank += (L.ms[j] > v) || (L.ms[j] == v && j < i);
        if (rank < nb) L.sel_hyp[rank] = i;
    }
    __syncthreads();
    if (tid < nb) {
        const int j = tid, r = b * nb + j;
        const int i = L.sel_hyp[j];
        float h;
        int fin, ht, hb, hk;
        if (i < nb) {
            h = L.o_hyp[i]; fin = L.o_fin[i]; ht = L.o_t[i]; hb = L.o_beam[i]; hk = L.o_tok[i];
        } else {
            const int k = i - nb;
            h = L.fs[k]; fin = L.hit[k] && k < nb; ht = t; hb = L.beam[k]; hk = L.tok[k];
        }
        L.n_hyp[j] = h;
        L.n_fin[j] = fin;
        S.hyp[r] = h; S.fin[r] = fin; S.hyp_t[r] = ht; S.hyp_beam[r] = hb; S.hyp_tok[r] = hk;
        const int k = L.sel_run[j];
        S.run[r] = L.rs[k];
        S.rtok[(int64_t)r * a.T + t] = L.tok[k];
        S.rpar[(int64_t)r * a.T + t] = L.beam[k];
        S.par[r] = b * nb + L.beam[k];
        a.tok[r] = L.tok[k];
        if (a.advance) {
            a.posid[r] += 1;
            if (r == 0) a.pos[0] += 1;
        }
    }
    __syncthreads();
    if (tid == 0) {
        // early-stop heuristic with cur_len advanced
        const int bl = (a.early_stopping == 2 && a.length_penalty > 0.f) ? a.max_new : t + 1;
        const float bp = L.rs[L.sel_run[0]] * (1.0f / (float)pow((double)bl, (double)a.length_penalty));
        float mn = L.n_hyp[0];
        int allfin = 1;
        for (int j = 0; j < nb; ++j) { mn = fminf(mn, L.n_hyp[j]); allfin &= L.n_fin[j] != 0; }
        int any = 0;
        for (int j = 0; j < nb; ++j) any |= bp > (L.n_fin[j] ? mn : NEG);
        F[nxt] = L.heur && any;
        F[nxt + 1] = allfin;
        F[nxt + 2] = L.allhit;
        F[3] = t + 1;
    }
}

constexpr int RE_THREADS = 256, RE_PER = 8;

__global__ __launch_bounds__(RE_THREADS) void beam_kv_reorder_kernel(const int64_t *__restrict__ ptrs, int B, int nb, int nkv, int maxlen, int D,
                                                                      const int *__restrict__ par, const int64_t *first_slot, int from_first,
                                                                      const int64_t *pos, int CH) {
    __shared__ int P[16];
    __shared__ int moved;
    int y = blockIdx.y;
    const int h = y % nkv;
    y /= nkv;
    const int b = y % B, ti = y / B;
    const int hi = (int)min((int64_t)maxlen, *pos);
    const int first = (int)max((int64_t)0, *first_slot);
    const int s0 = first + blockIdx.x * CH, s1 = min(s0 + CH, hi);
    if (s0 >= s1) return;
    if (threadIdx.x == 0) moved = 0;
    __syncthreads();
    if (threadIdx.x < nb) {
        const int p = from_first ? 0 : par[b * nb + threadIdx.x] - b * nb;
        P[threadIdx.x] = p;
        if (p != (int)threadIdx.x) atomicOr(&moved, 1);
    }
    __syncthreads();
    if (!moved) return;                               // identity parents: nothing moves
    bf16_t *base = (bf16_t *)ptrs[ti];
    const int dv = D / 8, ns = s1 - s0, per_beam = ns * dv, total = nb * per_beam;
    const int64_t row_elems = (int64_t)nkv * maxlen * D;
    uint4 v[RE_PER];
#pragma unroll
    for (int c = 0; c < RE_PER; ++c) {
        const int e = threadIdx.x + c * RE_THREADS;
        if (e < total) {
            const int j = e / per_beam, rem = e - j * per_beam, s = s0 + rem / dv, d = rem % dv;
            if (P[j] != j) {
                v[c] = *(const uint4 *)(base + (int64_t)(b * nb + P[j]) * row_elems + ((int64_t)h * maxlen + s) * D + d * 8);
                asm volatile("" : : "v"(v[c].x), "v"(v[c].y), "v"(v[c].z), "v"(v[c].w));     // loaded before the barrier
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < RE_PER; ++c) {
        const int e = threadIdx.x + c * RE_THREADS;
        if (e < total) {
            const int j = e / per_beam, rem = e - j * per_beam, s = s0 + rem / dv, d = rem % dv;
            if (P[j] != j) *(uint4 *)(base + (int64_t)(b * nb + j) * row_elems + ((int64_t)h * maxlen + s) * D + d * 8) = v[c];
        }
    }
}

}  // namespace
}  // namespace ll

using namespace ll;

extern "C" int64_t ll_beam_state_bytes(int B, int nb, int K, int T) {
    return (B <= 0 || nb <= 0 || K <= 0 || T <= 0) ? 0 : 4 * state_words(B, nb, K, T);
}

extern "C" int ll_beam_step_bf16(const void *logits, int64_t ld, int B, int nb, int V, int K, int T, void *state, int64_t state_bytes,
                                 const int64_t *eos, int n_eos, int max_new, float length_penalty, int early_stopping, int do_sample,
                                 float inv_temp, int top_k, float top_p, const int64_t *seed, int64_t *tok, int64_t *posid, int64_t *pos,
                                 int advance, void *stream) {
    LL_CHECK(logits && state && tok && (n_eos == 0 || eos) && (!advance || (posid && pos)) && (!do_sample || seed),
             "ll_beam_step_bf16: null argument");
    const int min_keep = n_eos ? n_eos + 1 : 2;
    LL_CHECK(B >= 1 && nb >= 2 && nb <= 16 && V >= 8 && V % 8 == 0 && V <= 163840 && ld % 8 == 0 && ld >= V,
             "ll_beam_step_bf16: need 2 <= nb <= 16, V %% 8 == 0, V <= 163840 (B=%d nb=%d V=%d)", B, nb, V);
    LL_CHECK(n_eos >= 0 && n_eos <= 32 && K == (n_eos + 1 > 2 ? n_eos + 1 : 2) * nb && K <= 512 && nb * K <= ITEM_CAP && K <= V,
             "ll_beam_step_bf16: K must be max(2, 1 + n_eos) * nb <= 512 with nb * K <= 4096 and n_eos <= 32 (K=%d)", K);
    LL_CHECK(max_new >= 1 && T >= max_new && early_stopping >= 0 && early_stopping <= 2, "ll_beam_step_bf16: bad max_new / T / early_stopping");
    LL_CHECK(!do_sample || (top_k >= 1 && (top_k > min_keep ? top_k : min_keep) <= 512 && inv_temp > 0.f && top_p >= 0.f),
             "ll_beam_step_bf16: beam sample needs 1 <= top_k, max(top_k, n_eos + 1) <= 512 and a positive temperature");
    LL_CHECK(state_bytes >= ll_beam_state_bytes(B, nb, K, T) && ((uintptr_t)state & 15) == 0, "ll_beam_step_bf16: state too small or misaligned");
    hipStream_t s = (hipStream_t)stream;
    RowArgs ra{(const bf16_t *)logits, ld, B, nb, V, K, T, state, do_sample, top_k, min_keep, inv_temp, top_p, seed};
    hipLaunchKernelGGL(beam_rows_kernel, dim3(B * nb), dim3(ROW_THREADS), 0, s, ra);
    LL_LAUNCH_CHECK();
    ItemArgs ia{B, nb, V, K, T, state, eos, n_eos, max_new, length_penalty, early_stopping, tok, posid, pos, advance};
    hipLaunchKernelGGL(beam_item_kernel, dim3(B), dim3(ITEM_THREADS), 0, s, ia);
    LL_LAUNCH_CHECK();
    return LL_OK;
}

extern "C" int ll_beam_kv_reorder_bf16(const int64_t *kv_ptrs, int n_tensors, int B, int nb, int nkv, int maxlen, int D, const int *par,
                                       const int64_t *first, int from_first_beam, const int64_t *pos, void *stream) {
    LL_CHECK(kv_ptrs && pos && first && (from_first_beam || par), "ll_beam_kv_reorder_bf16: null argument");
    LL_CHECK(n_tensors >= 1 && B >= 1 && nb >= 2 && nb <= 16 && nkv >= 1 && maxlen >= 1 && D >= 8 && D % 8 == 0 && nb * (D / 8) <= RE_THREADS * RE_PER
             && (int64_t)n_tensors * B * nkv <= 65535,
             "ll_beam_kv_reorder_bf16: need 2 <= nb <= 16, D %% 8 == 0, nb * D <= 16384 (nb=%d D=%d)", nb, D);
    // first and *pos are read on the device (a captured launch serves calls of any prompt length): the grid covers every slot and the
    // chunks outside [first, *pos) return at once
    const int CH = RE_THREADS * RE_PER / (nb * (D / 8));
    hipLaunchKernelGGL(beam_kv_reorder_kernel, dim3(cdiv(maxlen, CH), n_tensors * B * nkv), dim3(RE_THREADS), 0, (hipStream_t)stream,
                       kv_ptrs, B, nb, nkv, maxlen, D, par, first, from_first_beam, pos, CH);
    LL_LAUNCH_CHECK();
    return LL_OK;
}
