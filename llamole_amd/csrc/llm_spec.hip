// Prompt-lookup speculative decoding of the graphed batch-1 decode (llamole_amd/llm_spec.py states the step in torch; HF reaches the same
// drafting rule through generate(prompt_lookup_num_tokens=k, max_matching_ngram_size=n), generation/candidate_generator.py
// PromptLookupCandidateGenerator.get_candidates).  One step = the model forward over S = k + 1 tokens [last emitted, d_1..d_k] of ONE
// sequence, then
//   * ll_spec_verify_bf16, two launches: (1) S workgroups of the token sampler (llm_sample.hip, sample_rows_spec: logits row i drawn as the
//     plain decode draws its row at step value t + i), (2) one workgroup that accepts the leading drafts the model agrees with, emits
//     x_0..x_a, does the loop's bookkeeping and -- as its tail, with draft_next -- writes the NEXT step's input rows;
//   * ll_spec_draft, one launch of one workgroup: the same drafting function on its own, for the first step of a call (it also appends the
//     token sampled from the prefill logits to the history).
// The tail was chosen over a third launch per step: the draft scans a history of a few thousand int64 (tens of KB, L2-resident) and is
// far below one launch gap.  Everything is plain C++ on vector stores; no host sync.
#include <limits.h>

#include "common.h"

namespace ll {

constexpr int SPEC_THREADS = 1024;
constexpr int SPEC_MIN_ROWS = 3, SPEC_MAX_ROWS = 16;       // the rows the fused query-token forward serves

// The drafting rule on hist[0, L) (the call's input_ids row, then every emitted token): ngram sizes min(n, L - 1) down to 1; the LEFTMOST
// earlier occurrence of the history's last ngram that has a non-empty continuation (start idx with idx + ng < L); the drafts are the up to
// k tokens behind it.  Row 0 is the last emitted token, rows without a draft repeat it (a valid id).  Also the rows' position ids
// posid + i and cache positions pos + i.  Called by all SPEC_THREADS threads of one workgroup; sh_best is one int of LDS.
__device__ __forceinline__ void spec_draft_rows(const long long *__restrict__ hist, int L, int k, int n, long long last, long long pos,
                                                long long posid, long long *__restrict__ ids, long long *__restrict__ position_ids,
                                                long long *__restrict__ cache_position, int *sh_best, int tid) {
    int best = INT_MAX, ngf = 0;
    for (int ng = min(n, L - 1); ng >= 1; --ng) {
        if (tid == 0) *sh_best = INT_MAX;
        __syncthreads();
        int mine = INT_MAX;
        for (int idx = tid; idx + ng < L; idx += SPEC_THREADS) {      // ascending: the first hit is this thread's leftmost
            bool m = true;
            for (int j = 0; j < ng && m; ++j) m = hist[idx + j] == hist[L - ng + j];
            if (m) { mine = idx; break; }
        }
        if (mine != INT_MAX) atomicMin(sh_best, mine);
        __syncthreads();
        best = *sh_best;
        __syncthreads();
        if (best != INT_MAX) { ngf = ng; break; }
    }
    if (tid <= k) {
        long long t = last;
        if (tid >= 1 && best != INT_MAX) {
            const int src = best + ngf + tid - 1;
            if (src < L) t = hist[src];
        }
        ids[tid] = t;
        position_ids[tid] = posid + tid;
        cache_position[tid] = pos + tid;
    }
}

__device__ __forceinline__ int spec_len(const long long *hist_len, int cap) {
    const long long l = *hist_len;
    return l < 0 ? 0 : (l > cap ? cap : (int)l);
}

__global__ __launch_bounds__(SPEC_THREADS) void spec_draft_kernel(long long *hist, int cap, long long *hist_len, const long long *tok, int append,
                                                                  int k, int n, const long long *pos, const long long *posid, long long *ids,
                                                                  long long *position_ids, long long *cache_position) {
    __shared__ int sh_best, sh_L;
    const int tid = threadIdx.x;
    if (tid == 0) {
        int L = spec_len(hist_len, cap);
        if (append && L < cap) {
            hist[L++] = *tok;
            *hist_len = L;
        }
        sh_L = L;
    }
    __syncthreads();          // the appended token is visible to the workgroup
    spec_draft_rows(hist, sh_L, k, n, *tok, *pos, *posid, ids, position_ids, cache_position, &sh_best, tid);
}

struct SpecArgs {
    const long long *xs;       // [S] the sampled tokens of the S logits rows
    int S;
    const long long *eos;
    int n_eos;
    unsigned char *done;       // [1]
    long long *tok;            // [1] the last emitted token = row 0 of the next forward
    long long *out_tokens;     // [out_cap], column step
    int out_cap;
    const long long *max_new;  // [1] device: a captured step serves every max_new_tokens of its cache bucket
    long long *step, *posid, *pos;     // [1] each
    long long *cumulative_length;      // [1] or null: layer 0's counter of a fused cache, set to the new pos
    long long *ids, *position_ids, *cache_position;    // [S]: in, ids[1..k] the drafts that were forwarded; out (draft_next), the next step's rows
    long long *hist;
    int cap;
    long long *hist_len;
    int n, draft_next;
    long long *stats;          // [2] forwards, accepted
};

__global__ __launch_bounds__(SPEC_THREADS) void spec_accept_kernel(SpecArgs a) {
    __shared__ int sh_best, sh_L, sh_go;
    const int tid = threadIdx.x, k = a.S - 1;
    if (tid == 0) {
        int go = 0, L = spec_len(a.hist_len, a.cap);
        const long long t = a.step[0];
        const long long lim = *a.max_new < (long long)a.out_cap ? *a.max_new : (long long)a.out_cap;
        if (!a.done[0] && t >= 0 && t < lim) {           // a step after done, or after step == max_new, changes nothing
            int e = 0;
            bool stop = false;
            long long last = 0;
            for (int i = 0; i <= k; ++i) {
                const long long x = a.xs[i];
                a.out_tokens[t + e] = x;
                if (L < a.cap) a.hist[L++] = x;
                last = x;
                ++e;
                for (int j = 0; j < a.n_eos; ++j) stop = stop || a.eos[j] == x;
                if (stop || t + e >= lim) break;
                if (i >= k || a.ids[i + 1] != x) break;   // x_i is the model's own token; the next row is valid only if it was drafted
            }
            a.step[0] = t + e;
            const long long np = a.pos[0] + e;
            a.pos[0] = np;
            a.posid[0] += e;
            if (a.cumulative_length) *a.cumulative_length = np;
            a.tok[0] = last;
            if (stop) a.done[0] = 1;
            *a.hist_len = L;
            a.stats[0] += 1;
            a.stats[1] += e - 1;
            go = a.draft_next;
        }
        sh_go = go;
        sh_L = L;
    }
    __syncthreads();          // the bookkeeping above is visible to the workgroup
    if (!sh_go) return;
    spec_draft_rows(a.hist, sh_L, k, a.n, a.tok[0], a.pos[0], a.posid[0], a.ids, a.position_ids, a.cache_position, &sh_best, tid);
}

}  // namespace ll

using namespace ll;

extern "C" int ll_spec_draft(int64_t *hist, int hist_cap, int64_t *hist_len, const int64_t *tok, int append, int k, int n, const int64_t *pos,
                             const int64_t *posid, int64_t *ids, int64_t *position_ids, int64_t *cache_position, void *stream) {
    LL_CHECK(hist && hist_len && tok && pos && posid && ids && position_ids && cache_position, "ll_spec_draft: null argument");
    LL_CHECK(k + 1 >= SPEC_MIN_ROWS && k + 1 <= SPEC_MAX_ROWS, "ll_spec_draft: %d draft tokens, must be 2..15 (3..16 rows)", k);
    LL_CHECK(n >= 1 && hist_cap >= 1, "ll_spec_draft: ngram size %d and history capacity %d must be >= 1", n, hist_cap);
    hipLaunchKernelGGL(spec_draft_kernel, dim3(1), dim3(SPEC_THREADS), 0, (hipStream_t)stream, (long long *)hist, hist_cap, (long long *)hist_len,
                       (const long long *)tok, append, k, n, (const long long *)pos, (const long long *)posid, (long long *)ids,
                       (long long *)position_ids, (long long *)cache_position);
    LL_LAUNCH_CHECK();
    return LL_OK;
}

extern "C" int ll_spec_verify_bf16(const void *logits, int64_t ld, int S, int V, float inv_temp, float top_p, int top_k, int greedy,
                                   const int64_t *seed, const int64_t *eos, int n_eos, void *done, int64_t *tok, int64_t *out_tokens, int out_cap,
                                   const int64_t *max_new, int64_t *step, int64_t *posid, int64_t *pos, int64_t *cumulative_length, int64_t *ids,
                                   int64_t *position_ids, int64_t *cache_position, int64_t *hist, int hist_cap, int64_t *hist_len, int n,
                                   int draft_next, int64_t *stats, int64_t *xs, void *stream) {
    LL_CHECK(logits && seed && done && tok && out_tokens && max_new && step && posid && pos && ids && position_ids && cache_position && hist &&
                 hist_len && stats && xs && (n_eos == 0 || eos),
             "ll_spec_verify_bf16: null argument");
    LL_CHECK(S >= SPEC_MIN_ROWS && S <= SPEC_MAX_ROWS, "ll_spec_verify_bf16: %d rows, must be 3..16", S);
    LL_CHECK(V >= 8 && V % 8 == 0 && V <= 1024 * 8 * 20 && ld % 8 == 0 && ld >= V && ((uintptr_t)logits & 15) == 0,
             "ll_spec_verify_bf16: vocabulary %d must be a multiple of 8 and <= 163840, the rows 16-byte aligned", V);
    LL_CHECK(greedy || (inv_temp > 0.f && top_p >= 0.f), "ll_spec_verify_bf16: temperature and top_p must be positive");
    LL_CHECK(n_eos >= 0 && n >= 1 && hist_cap >= 1 && out_cap >= 1, "ll_spec_verify_bf16: n_eos %d, ngram size %d, capacities %d / %d", n_eos, n,
             hist_cap, out_cap);
    hipStream_t s = (hipStream_t)stream;
    LL_TRY(sample_rows_spec(logits, ld, S, V, inv_temp, top_p, top_k, greedy, seed, step, xs, s));
    SpecArgs a;
    a.xs = (const long long *)xs; a.S = S; a.eos = (const long long *)eos; a.n_eos = n_eos; a.done = (unsigned char *)done;
    a.tok = (long long *)tok; a.out_tokens = (long long *)out_tokens; a.out_cap = out_cap; a.max_new = (const long long *)max_new;
    a.step = (long long *)step; a.posid = (long long *)posid; a.pos = (long long *)pos; a.cumulative_length = (long long *)cumulative_length;
    a.ids = (long long *)ids; a.position_ids = (long long *)position_ids; a.cache_position = (long long *)cache_position;
    a.hist = (long long *)hist; a.cap = hist_cap; a.hist_len = (long long *)hist_len; a.n = n; a.draft_next = draft_next;
    a.stats = (long long *)stats;
    hipLaunchKernelGGL(spec_accept_kernel, dim3(1), dim3(SPEC_THREADS), 0, s, a);
    LL_LAUNCH_CHECK();
    return LL_OK;
}
