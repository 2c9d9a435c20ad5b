/*
 * llamole_hip.h -- C ABI of the MI355X (gfx950) implementation of Llamole's graph hot path.
 *
 * The reference (liugangcode/Llamole) has NO native/FFI interface: its seam is the Python
 * class level.  This header is therefore the boundary a maintainer
 * would bind from Python with ctypes; every entry point cites the
 * reference Python interface it replaces.  Conventions:
 *   - plain pointers and sizes only; all data pointers are DEVICE pointers unless named h_*;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); calls are asynchronous
 *     on that stream unless stated otherwise;
 *   - every function returns 0 on success or a negative LL_E* code; the message is available
 *     through ll_last_error() (thread-local).  No C++ exception crosses the boundary;
 *   - one in-flight call per handle; handles are independent of each other.
 */
#ifndef LLAMOLE_HIP_H
#define LLAMOLE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LL_OK 0
#define LL_EINVAL (-1)   /* bad argument / unsupported shape */
#define LL_EHIP (-2)     /* a HIP runtime call failed        */
#define LL_ESTATE (-3)   /* call order violated              */

#define LL_F32 0
#define LL_BF16 1

#define LL_XDIM 16       /* atom classes   (reference diffusion_utils.py:58-59) */
#define LL_EDIM 5        /* bond classes                                          */
#define LL_YDIM 10       /* property slots                                        */
#define LL_TEXT_DIM 768  /* text-embedding width (diffusion_model.py:62)          */

int ll_version(void);
const char *ll_last_error(void);

/* ------------------------------------------------------------------ dense linear (building block)
 * C[M,N] = epi(A[M,K] * W[N,K]^T + bias)   -- torch.nn.Linear layout, used by every Linear on the
 * path (reference layers.py:47,53,106-109; transformer.py:116-130).  dtype selects the operand type
 * of A and W (LL_F32: exact f32 FMA chains; LL_BF16: MFMA 16x16x32 with f32 accumulation).
 * epi: 0 none, 1 GELU(erf), 2 SiLU, 3 Softsign.  out_f32 != 0 writes f32, else the operand dtype.
 * bf16: M <= 4 runs a weight-streaming GEMV, larger M the LDS-DMA pipelined MFMA tiles (A rows are clamped, no
 * padding needed); f32: A must be readable for round_up(M,64) rows. */
int ll_linear(int dtype, const void *A, int lda, const void *W, int ldw, const float *bias, void *C, int ldc,
              int M, int N, int K, int epi, int out_f32, void *stream);

/* bf16 Linear with the K dimension split over `splits` workgroup groups (2..16, K % (64*splits) == 0): for a few rows times a
 * short, wide weight matrix (batch-8/16 decode through down_proj: 3584 x 18944) an unsplit launch has too few workgroups to
 * pull HBM bandwidth.  workspace: device f32 [splits * M * N]; partial slabs are summed in order (deterministic). */
int ll_linear_splitk_bf16(const void *A, int lda, const void *W, int ldw, const float *bias, void *C, int ldc, int M, int N,
                          int K, int epi, int splits, float *workspace, void *stream);


/* ------------------------------------------------------------------ GraphDiT sampler
 * Replaces reference GraphDiT.generate / sample_p_zs_given_zt / Transformer.forward
 * (src/model/graph_decoder/diffusion_model.py:252-399, transformer.py:93-187,
 *  diffusion_utils.py:273-349,376-413,476-518). */
/* Any sizes the reference Transformer constructs are valid (transformer.py:24-37): hidden, heads (dividing hidden) and mlp_hidden need
 * not be multiples of anything -- the engine zero-pads its internal copy of the weights to row pitches of 64 and a head pitch of 32 and
 * takes the true widths for every row statistic; the arena layout below is the checkpoint's own.  Bounds (LL_EINVAL beyond them):
 * hidden <= 2048, hidden / heads <= 128, max_nodes <= 128 (65..128 nodes: two wavefronts per row of bond partners, a 128-row attention tile). */
typedef struct LLDitConfig {
    int hidden;        /* H            (config.yaml hidden_size)      */
    int depth;         /* L            (depth)                        */
    int heads;         /* num_heads                                    */
    int mlp_hidden;    /* int(H * mlp_ratio)                           */
    int max_nodes;     /* N            (data.meta.json max_node)       */
    int T;             /* diffusion_steps                              */
    float guide_scale; /* classifier-free guidance scale (1 = off)     */
    int dtype;         /* LL_F32 | LL_BF16: operand type of the Linears */
} LLDitConfig;

/* Host-side tables built from data.meta.json exactly as the reference does
 * (diffusion_model.py:78-103, diffusion_utils.py:172-187). */
typedef struct LLDitTables {
    const float *h_x_marg;     /* [16]     */
    const float *h_e_marg;     /* [5]      */
    const float *h_u_xe;       /* [16*5]   row-normalised S            */
    const float *h_u_ex;       /* [5*16]   row-normalised S^T          */
    const float *h_betas;      /* [T+1]    */
    const float *h_alphas_bar; /* [T+1]    */
} LLDitTables;

/* Weight arena layout: parameters in the order of the reference Transformer.state_dict()
 * (SURVEY.md section 8b).  idx in [0, ll_dit_param_count).  offset/numel in f32 elements. */
int ll_dit_param_count(const LLDitConfig *cfg);
int ll_dit_param_info(const LLDitConfig *cfg, int idx, char *name, int name_cap, int64_t *numel, int64_t *offset);
int64_t ll_dit_arena_elems(const LLDitConfig *cfg);

/* d_weights_f32: device arena laid out as above (f32 masters; converted once to cfg->dtype). Synchronous. */
int ll_dit_create(const LLDitConfig *cfg, const LLDitTables *tables, const float *d_weights_f32, void **handle);
int ll_dit_destroy(void *handle);

/* Start a batch (GraphDiT.generate up to the loop, diffusion_model.py:259-268; conditions.py:19-123):
 * properties [B,10] (NaN = absent), text [B,768] (a NaN in a row drops the row), n_nodes [B] int32.
 * Hoists every step-invariant piece out of the T-step loop: c = c_t + c_y + c_txt for all T steps and
 * all L+1 adaLN modulations (transformer.py:125-130,156-160). */
int ll_dit_begin(void *handle, int B, const float *props, const float *text, const int32_t *n_nodes, void *stream);

/* z_T ~ limit marginals (diffusion_utils.py:495-518).  qx [B*N,16], qe [B*N*N,5] = Exp(1) race noise in the
 * reference's draw order, or NULL/NULL to draw on device from Philox4x32-10(seed). */
int ll_dit_init_state(void *handle, const float *qx, const float *qe, uint64_t seed, void *stream);

/* One reverse step z_{s+1} -> z_s (sample_p_zs_given_zt, diffusion_model.py:309-399), s in [0,T). */
int ll_dit_step(void *handle, int s, const float *qx, const float *qe, uint64_t seed, void *stream);

/* Whole trajectory T-1 .. 0 with on-device noise.  use_graph: 1 = the step is captured once as a hipGraph (five steps per graph when
 * that divides T) and replayed -- the host call returns at once; 0 = every kernel launched from this call's loop (no Python in it) --
 * measured 4-14 % faster per step than the replay when the trajectory has the GPU to itself (consecutive kernel nodes of a replayed
 * graph start ~1.8 us apart at best, consecutive queued launches ~1.3 us), but the host is busy for most of the trajectory's duration
 * (~4 us per launch); 2 = the library's choice: launches when the engine is not in overlap mode, the replay when it is (the host then
 * has the next prompt's LLM decode to feed); the environment variable LL_DIT_RUN_MODE = graph | launches overrides that choice. */
enum { LL_DIT_RUN_LAUNCHES = 0, LL_DIT_RUN_GRAPH = 1, LL_DIT_RUN_AUTO = 2 };
int ll_dit_run(void *handle, uint64_t seed, int use_graph, void *stream);

/* State I/O: X int8 [B,N] (-1 = masked), E int8 [B,N,N] (-1 = all-zero one-hot: masked pair or z_T diagonal). */
int ll_dit_set_state(void *handle, const int8_t *X, const int8_t *E, void *stream);
int ll_dit_get_state(void *handle, int8_t *X, int8_t *E, void *stream);

/* Parity taps (tests only): run the denoiser on the current state at step s.
 * logX [2,B,N,16], logE [2,B,N,N,5] (pass 0 = conditional, 1 = unconditional), masked like
 * Transformer.forward's PlaceHolder.mask; hidden (nullable) [2,B,N,H] = residual stream after `tap_layer`
 * blocks (0 = after x_embedder). */
int ll_dit_denoise(void *handle, int s, float *logX, float *logE, float *hidden, int tap_layer, void *stream);
/* Guided probabilities of step s as handed to sample_discrete_features: pX [B,N,16], pE [B,N,N,5]
 * (only rows of valid nodes / pairs i<j of valid nodes are defined; others are written as 0). */
/* ll_dit_denoise_rows : the denoiser's conditional / unconditional logits for the current state (ll_dit_set_state) with a
 * PER-GRAPH timestep t_int[b] in 0..T (device int32 [B]) instead of one shared reverse step: the training forward
 * (GraphDiT.forward / apply_noise, diffusion_model.py:148-250) draws t independently per graph, t = 0 included.
 * logX [2][B][N][16], logE [2][B][N][N][5] as ll_dit_denoise. */
int ll_dit_denoise_rows(void *handle, const int32_t *t_int, float *logX, float *logE, void *stream);
int ll_dit_step_probs(void *handle, int s, float *pX, float *pE, void *stream);
/* Conditioning vectors c [B+1,H] at step s (rows 0..B-1 conditional, row B unconditional). */
int ll_dit_cvec(void *handle, int s, float *c, void *stream);

/* Timing of the most recent ll_dit_run measured with HIP events on `stream`: total ms and steps. */
/* ll_dit_set_overlap : on = the next ll_dit_run trajectories run NEXT TO another stream's kernels (GraphDiT.generate_graphs_async
 *     under the LLM decode of the next prompt): their <= 64-row panel GEMMs take the 48 KB LDS-DMA ring instead of the panel kernel,
 *     whose workgroups need a whole CU's LDS (slower alone, faster for the pair); a separate captured step is kept per mode. */
int ll_dit_set_overlap(void *handle, int on);
/* ll_dit_set_option : per-engine switches, effective for every later denoiser call of this handle (step / run / denoise /
 * step_probs).  LL_DIT_OPT_OVERLAP = ll_dit_set_overlap; LL_DIT_OPT_GENERIC_ATTN = run the f32-LDS attention kernel under the
 * bf16 engine instead of the MFMA one (parity hook: the two are compared on identical q|k|v by the tests);
 * LL_DIT_OPT_FUSED_QKV_ATTN = the block's q|k|v projection and attention as ONE launch per (sequence, head) (bf16, head
 * dimension 64, hidden 256 | 512 | a multiple of 1024): -1 = above 128 token rows when the launch has 64..512 such workgroups, i.e. batch 3..16
 * at 16 heads and 32 nodes -- two sequences per workgroup from batch 11 to 24 -- and always in overlap mode (default), 0 = never,
 * 1 = whenever eligible, 2 = two sequences per workgroup whenever eligible (graphs of <= 32 nodes).
 * The launch chain is the one GraphDiT step this library has: the per-XCD persistent trajectory kernel, the per-XCD projection + AdaLN
 * launch and the packed-weight panel MLP GEMM of rounds 2-4 were measured slower at every batch and have been removed (HISTORY.md). */
enum { LL_DIT_OPT_OVERLAP = 0, LL_DIT_OPT_GENERIC_ATTN = 1, LL_DIT_OPT_FUSED_QKV_ATTN = 2 };
int ll_dit_set_option(void *handle, int option, int value);
int ll_dit_last_run_ms(void *handle, float *ms, int *steps);
/* ------------------------------------------------------------------ GIN encoder / predictor
 * Replaces GNNEncoder.forward + ProjectionHead (src/model/graph_encoder/model.py:124-205) and
 * GNNRetrosynthsizer.forward (src/model/graph_predictor/model.py:306-353). */
/* hidden (<= 2048) and text_dim need not be multiples of 64 either: zero-padded inside the engine (graph_encoder/model.py:87-112,
 * graph_predictor/model.py:231-278 take them from the checkpoint's config); out_dim is any positive number of templates. */
typedef struct LLGinConfig {
    int num_layer;
    int hidden;     /* H_gin                                   */
    int kind;       /* 0 = encoder (+projection head), 1 = predictor (+decoder) */
    int out_dim;    /* predictor: #templates (num_task); encoder: ignored          */
    int text_dim;   /* predictor: 768                                              */
    int dtype;      /* LL_F32 | LL_BF16                                            */
} LLGinConfig;

int ll_gin_param_count(const LLGinConfig *cfg);
int ll_gin_param_info(const LLGinConfig *cfg, int idx, char *name, int name_cap, int64_t *numel, int64_t *offset);
int64_t ll_gin_arena_elems(const LLGinConfig *cfg);
int ll_gin_create(const LLGinConfig *cfg, const float *d_weights_f32, void **handle);
int ll_gin_destroy(void *handle);

/* x [n] atom ids in [0,118).  Edges in CSR-by-destination form: rowptr [n+1], and for e in
 * [rowptr[v], rowptr[v+1]) the message source src[e] and bond class attr[e] in 0..4 (the PyG
 * edge_index[0] / edge_attr of the edges whose edge_index[1] == v, in stable order).
 * batch [n] sorted graph ids, gptr [G+1] node offsets of each graph.
 * c [G,text_dim] or NULL (predictor: NULL -> text_dropping row, model.py:315-316).
 * out: encoder [G,H] L2-normalised embedding; predictor [G,out_dim] template logits.
 * pooled (nullable) [G,H]: add-pooled node states before the head. */
/* ll_graph_csr : the reference's graph batch (int64 x [n], edge_index [2,E], edge_attr [E], sorted batch [n]; modeling_llamole.py:
 * 328-333, 611-616, 829-834) -> the int32 arrays of ll_gin_forward in one launch: x32 [n], rowptr [n+1] / src [E] / attr [E] =
 * CSR by destination with every node's in-edges in edge-list order (the reference's summation order), batch32 [n], gptr [G+1].
 * scratch: n int32.  *err (device memory, or pinned host memory so that the caller's stream never carries a read-back) = 0, 1 (batch
 * unsorted / graph id out of range), 2 (edge endpoint out of range) or 3 (atom type outside [0,118) / bond type outside [0,5)).  Whatever
 * the flag says the output arrays are in bounds for ll_gin_forward (ids clamped, bad edges dropped), so the caller may check it late. */
int ll_graph_csr(const int64_t *x, const int64_t *edge_index, const int64_t *edge_attr, const int64_t *batch, int n_nodes, int n_edges,
                 int n_graphs, int32_t *x32, int32_t *rowptr, int32_t *src, int32_t *attr, int32_t *batch32, int32_t *gptr,
                 int32_t *scratch, int32_t *err, void *stream);
int ll_gin_forward(void *handle, const int32_t *x, const int32_t *rowptr, const int32_t *src, const int32_t *attr,
                   const int32_t *batch, const int32_t *gptr, int n_nodes, int n_edges, int n_graphs, const float *c,
                   float *out, float *pooled, void *stream);

/* Training path of the predictor (reference modeling_llamole.py:385-419: the retro cross-entropy
 * reaches the LLM through c = lm_to_graph_predictor(hidden); the predictor's own weights are frozen):
 * ll_gin_forward_train = ll_gin_forward (predictor, c != NULL) that also keeps the per-layer activations;
 * ll_gin_backward_c    = d loss / d c [G,text_dim] from d loss / d logits [G,out_dim] for the batch of the last
 *                        ll_gin_forward_train call (LL_ESTATE otherwise).  Edges here in CSR-by-SOURCE form: rowptr_src [n+1],
 *                        and for e in [rowptr_src[v], rowptr_src[v+1]) the message destination dst[e] and bond class attr[e].
 * Replaces torch.autograd through GNNRetrosynthsizer.forward (graph_predictor/model.py:306-353). */
int ll_gin_forward_train(void *handle, const int32_t *x, const int32_t *rowptr, const int32_t *src, const int32_t *attr,
                         const int32_t *batch, const int32_t *gptr, int n_nodes, int n_edges, int n_graphs, const float *c,
                         float *out, void *stream);
int ll_gin_backward_c(void *handle, const int32_t *rowptr_src, const int32_t *dst, const int32_t *attr, const int32_t *batch,
                      const int32_t *gptr, int n_nodes, int n_edges, int n_graphs, const float *c, const float *dlogits, float *dc,
                      void *stream);

/* softmax over out_dim then top-k (GraphPredictor.sample_templates, graph_predictor/model.py:174-179).
 * probs [rows,k] descending, idx [rows,k]. k <= 64. */
int ll_softmax_topk(const float *logits, int rows, int out_dim, int k, float *probs, int32_t *idx, void *stream);

/* CostMLP (graph_predictor/model.py:356-391): softplus(W3 relu(W0 fp + b0) + b3); fps [n,2048] f32 0/1.
 * weights: device f32 arena = [layers.0.weight 128x2048 | layers.0.bias 128 | layers.3.weight 1x128 | layers.3.bias 1]. */
int ll_cost_mlp(const float *weights, const float *fps, int n, float *out, void *stream);

/* ------------------------------------------------------------------ fused LLM decode helpers (optional, section 8 f2)
 * Same arithmetic as the HuggingFace modules they stand in for, including the intermediate bf16 roundings of PyTorch's
 * op-by-op evaluation (results are bit-identical); all tensors bf16.
 * ll_rmsnorm_bf16 : Qwen2RMSNorm/LlamaRMSNorm.forward on [rows,H].
 * ll_rope_bf16    : apply_rotary_pos_emb on q [B,nh,S,D] / k [B,nkv,S,D] given by element strides of dims 0..2 (last dim
 *                   contiguous) and cos/sin [B or 1,S,D] strides of dims 0..1; outputs contiguous.
 * ll_silu_mul_bf16: silu(gate) * up on [rows, cols] views with input row stride ld_in (elements), contiguous output. */
int ll_rmsnorm_bf16(const void *x, const void *w, void *out, int rows, int H, float eps, void *stream);
int ll_rope_bf16(const void *q, const void *k, const void *cos, const void *sin, void *qo, void *ko, int B, int nh, int nkv,
                 int S, int D, const int64_t *qstr, const int64_t *kstr, const int64_t *cstr, void *stream);
int ll_silu_mul_bf16(const void *gate, const void *up, void *out, int rows, int cols, int64_t ld_in, void *stream);
/* ll_kv_append_bf16 : StaticCache layer update at decode: write k_new/v_new [B,nkv,S,D] (element strides of dims 0..2) into
 *                     keys/values [B,nkv,maxlen,D] at positions *pos .. *pos+S-1 (pos: device int64).
 * ll_decode_attn_bf16: softmax(q K^T * scale + mask) V over the static cache with grouped-query heads; q [B,nh,S,D] strided,
 *                     mask bool [B,1,S,maxlen] (strides of dims 0 and 2), out [B,S,nh,D] contiguous; D in {64,128}, maxlen <= 16384
 *                     (LL_EINVAL beyond: a workgroup keeps the scores of all keys in LDS; longer caches: ll_decode_attn_rope_split_bf16 /
 *                     ll_suffix_attn_rope_split_bf16 below).  A query row without a visible key gives zeros. */
int ll_kv_append_bf16(void *K, void *V, const void *k_new, const void *v_new, const int64_t *pos, int B, int nkv, int S,
                      int maxlen, int D, const int64_t *kstr, const int64_t *vstr, void *stream);
int ll_decode_attn_bf16(const void *q, const void *K, const void *V, const void *mask, void *out, int B, int nh, int nkv, int S,
                        int maxlen, int D, float scale, const int64_t *qstr, const int64_t *mstr, void *stream);

/* ---- decode-step layer fusion (one decoder layer of the HF LLM at batch <= 4 = five launches) ----------------------------
 * ll_gemv_fused_bf16 : out[M,N] = epilogue( rmsnorm?(x)[M,K] . W^T + bias ), M in 1..4, bf16 operands, f32 accumulation.
 *     norm_w != NULL : x is first normalised like Qwen2RMSNorm/LlamaRMSNorm (K <= 8192, M*K <= 32768), eps as given;
 *     epi LL_GEMV_PLAIN    : bf16(acc + bias)                                 (nn.Linear; fused q/k/v; lm_head)
 *         LL_GEMV_RESIDUAL : bf16(residual + bf16(acc + bias))                (o_proj / down_proj + the layer's residual add)
 *         LL_GEMV_SILU_MUL : W has 2N rows (gate rows [0,N), up rows [N,2N)): bf16(bf16(silu(gate)) * up)   (gated MLP)
 *     Replaces <Model>RMSNorm.forward + nn.Linear.forward + the residual add / act_fn(gate)*up of
 *     transformers modeling_qwen2.py Qwen2DecoderLayer.forward / Qwen2MLP.forward (bit-identical arithmetic).
 * ll_decode_attn_rope_bf16 : apply_rotary_pos_emb + StaticLayer.update + attention for ONE new position per sequence.
 *     qkv [B, (nh+2*nkv)*D] rows (stride ld_qkv) = fused q|k|v projection; cos/sin [B or 1, D] (batch stride cs_stride, 0 to
 *     broadcast); Kc/Vc [B,nkv,maxlen,D] static cache, appended at *pos (device int64); mask bool [B,maxlen] rows
 *     (stride mask_stride) for the new query (causal decode: cache slots behind *pos hold no keys yet and must be masked -- with more than 16
 *     sequences, where one workgroup serves the whole KV group, they are not even fetched); out [B, nh*D].  D in {64,128},
 *     maxlen <= 16384 (LL_EINVAL beyond).
 * ll_decode_attn_rope_qkn_bf16 : the same for the Qwen3 layout, whose attention normalises every q head row and every k head row over
 *     head_dim (Qwen3RMSNorm q_norm / k_norm, transformers modeling_qwen3.py) between the projection and the rotary embedding.  Per head
 *     row x [D] of q (weights q_norm_w [D] bf16) and of k (k_norm_w [D] bf16), one eps for both:
 *         xh = bf16( x * rsqrt( mean_D(x^2) + eps ) )        mean, rsqrt and product in f32, ONE rounding to bf16
 *         y  = bf16( w * xh )                                f32 product of two bf16 values, ONE rounding to bf16
 *     and y takes the place of x in the rotary arithmetic above; v is not normalised.  Same choice between the per-head and the grouped
 *     kernel, same shape bounds.  NULL norm weights or eps <= 0: LL_EINVAL, nothing is launched.
 * (timing / tuning hooks of these kernels: include/llamole_hip_tuning.h) */
#define LL_GEMV_PLAIN 0
#define LL_GEMV_RESIDUAL 1
#define LL_GEMV_SILU_MUL 2
int ll_gemv_fused_bf16(const void *x, int ldx, const void *W, int ldw, const float *bias, const void *norm_w, float eps,
                       const void *residual, int ldr, void *out, int ldc, int M, int N, int K, int epi, void *stream);
int ll_decode_attn_rope_bf16(const void *qkv, int64_t ld_qkv, const void *cos, const void *sin, int64_t cs_stride, void *Kc,
                             void *Vc, const int64_t *pos, const void *mask, int64_t mask_stride, void *out, int B, int nh,
                             int nkv, int maxlen, int D, float scale, void *stream);
int ll_decode_attn_rope_qkn_bf16(const void *qkv, int64_t ld_qkv, const void *cos, const void *sin, int64_t cs_stride, void *Kc,
                                 void *Vc, const int64_t *pos, const void *mask, int64_t mask_stride, void *out, int B, int nh,
                                 int nkv, int maxlen, int D, float scale, const void *q_norm_w, const void *k_norm_w, float eps,
                                 void *stream);
/* ll_decode_prologue : per-token prologue of a decode step in one launch: cos/sin [B,D] bf16 of Qwen2RotaryEmbedding.forward
 *     (transformers modeling_qwen2.py: inv_freq * position in f32, cos/sin, * attention_scaling, cast) for position_ids [B],
 *     and the boolean key mask [B,maxlen] of create_causal_mask (masking_utils.py) for one new query at cache slot *pos:
 *     key j visible iff j <= *pos and mask2d[b][j] != 0 (mask2d int64, row stride mask_stride). */
int ll_decode_prologue(const int64_t *position_ids, const float *inv_freq, float attention_scaling, const int64_t *mask2d,
                       int64_t mask_stride, const int64_t *pos, void *cos, void *sin, void *mask_out, int B, int D, int maxlen,
                       void *stream);
/* ll_suffix_prologue / ll_suffix_attn_rope_bf16 : the same pair for S consecutive new positions per sequence -- the reference's query-token
 *     re-forward (modeling_llamole.py:641-646: <design_start> + the body tokens) run on top of the decode's KV cache at slots
 *     *pos .. *pos+S-1.  Rows r = b*S + s.  Prologue: cos/sin [B*S,D] for position_ids [B*S], key mask [B*S,maxlen]: key j visible to row
 *     (b,s) iff j <= *pos + s and mask2d[b][j] != 0.  Attention: qkv [B*S, (nh+2*nkv)*D] (row stride ld_qkv); rotary on q and k, the
 *     new keys / values stored to Kc/Vc [B,nkv,maxlen,D], softmax(q K^T * scale + mask) V over the cache -> out [B*S, nh*D]; bit for
 *     bit ll_rope_bf16 + ll_kv_append_bf16 + ll_decode_attn_bf16.  S <= 16, D in {64,128}, maxlen <= 16384 (LL_EINVAL beyond); rows whose
 *     slot *pos + s lies past the cache are not stored (ll_kv_append_bf16 drops them alike).
 *     ll_suffix_attn_rope_qkn_bf16 : ll_suffix_attn_rope_bf16 with the per-head q / k RMSNorm of ll_decode_attn_rope_qkn_bf16 (same formula, same
 *     two roundings, same device function) in front of the rotation of every q row and every new k row: a key it stores is bit for bit the key
 *     ll_decode_attn_rope_qkn_bf16 stores for the same row and position.  NULL norm weights or eps <= 0: LL_EINVAL, nothing is launched. */
int ll_suffix_prologue(const int64_t *position_ids, const float *inv_freq, float attention_scaling, const int64_t *mask2d,
                       int64_t mask_stride, const int64_t *pos, void *cos, void *sin, void *mask_out, int B, int S, int D, int maxlen,
                       void *stream);
int ll_suffix_attn_rope_bf16(const void *qkv, int64_t ld_qkv, const void *cos, const void *sin, void *Kc, void *Vc, const int64_t *pos,
                             const void *mask, void *out, int B, int S, int nh, int nkv, int maxlen, int D, float scale, void *stream);
int ll_suffix_attn_rope_qkn_bf16(const void *qkv, int64_t ld_qkv, const void *cos, const void *sin, void *Kc, void *Vc, const int64_t *pos,
                                 const void *mask, void *out, int B, int S, int nh, int nkv, int maxlen, int D, float scale,
                                 const void *q_norm_w, const void *k_norm_w, float eps, void *stream);
/* ---- the same two calls split over the keys (flash-decoding), for static caches of up to 131072 slots ---------------------------------
 * ll_decode_attn_rope_split_bf16 : the arguments and semantics of ll_decode_attn_rope_qkn_bf16 (q_norm_w = k_norm_w = NULL: no per-head norm,
 *     i.e. ll_decode_attn_rope_bf16; given: eps > 0), plus a device workspace.
 * ll_suffix_attn_rope_split_bf16 : likewise for ll_suffix_attn_rope_qkn_bf16 / ll_suffix_attn_rope_bf16 (S <= 16 new positions per sequence).
 *     Two launches per call, both with a geometry that depends on (B, S, nh, nkv, maxlen, D) only -- *pos is read on the device, nothing
 *     synchronises with the host, so a captured graph replays them at every position:
 *       1. partial: the keys are cut into ranges of 512 slots; one workgroup per (range, group of query heads on one KV head, query row) writes
 *          the maximum m, the sum of exponentials l and the un-normalised f32 output of its range to the workspace.  A group is all nh / nkv
 *          heads of a KV head when that is 2, 4 or 7 (a K / V row is fetched once per group, for every B), one head otherwise.  A range
 *          without a visible key costs its 512 mask bytes and contributes (m, l) = (-inf, 0).
 *       2. combine: out = sum_r exp(m_r - M) acc_r / sum_r exp(m_r - M) l_r with M = max_r m_r, ranges with m_r = -inf left out; ONE rounding
 *          to bf16.  A query row without a visible key gives exact zeros.  Masked slots may hold anything (NaN).
 *     No atomics; every sum has a fixed order: the result is deterministic.  LDS per workgroup does not depend on maxlen.
 *     Stored rows: the K / V rows written at *pos (.. *pos+S-1; rows past the last slot are dropped) are bit for bit the rows the entry points
 *     above store (same device function for the norm, same rotary roundings), so a cache may be filled by either.  Each row is stored by one
 *     workgroup; no workgroup reads slots *pos .. *pos+S-1 from the cache in this call: a workgroup whose range holds them rotates the new rows
 *     itself.  Like above, the mask decides what is seen.
 *     Bounds: D in {64,128}, nh % nkv == 0, 1 <= maxlen <= 131072 (also <= 16384, where the entry points above apply too), decode 1 <= B <= 64,
 *     suffix 1 <= S <= 16 and B*S <= 65535, ld_qkv % 8 == 0; workspace 16-byte aligned, workspace_bytes >= ll_attn_split_workspace_bytes.
 *     Beyond them LL_EINVAL (ll_attn_split_workspace_bytes: -1) and nothing is launched.
 * ll_attn_split_workspace_bytes : bytes of the workspace for these sizes (decode: S = 1): B*S*nh*ceil(maxlen/512)*(D+2) f32; its layout is
 *     private.  Calls on one stream may share one workspace. */
int64_t ll_attn_split_workspace_bytes(int B, int S, int nh, int nkv, int maxlen, int D);
int ll_decode_attn_rope_split_bf16(const void *qkv, int64_t ld_qkv, const void *cos, const void *sin, int64_t cs_stride, void *Kc, void *Vc,
                                   const int64_t *pos, const void *mask, int64_t mask_stride, void *out, int B, int nh, int nkv, int maxlen,
                                   int D, float scale, const void *q_norm_w, const void *k_norm_w, float eps, void *workspace,
                                   int64_t workspace_bytes, void *stream);
int ll_suffix_attn_rope_split_bf16(const void *qkv, int64_t ld_qkv, const void *cos, const void *sin, void *Kc, void *Vc, const int64_t *pos,
                                   const void *mask, void *out, int B, int S, int nh, int nkv, int maxlen, int D, float scale,
                                   const void *q_norm_w, const void *k_norm_w, float eps, void *workspace, int64_t workspace_bytes,
                                   void *stream);
/* ---- the key-split calls for sliding-window layers (Mistral-v0.1, Qwen2 / Qwen3 with use_sliding_window) ------------------------------------
 * ll_decode_attn_rope_win_bf16 : the arguments of ll_decode_attn_rope_split_bf16 with `int window` in front of the workspace.
 * ll_suffix_attn_rope_win_bf16 : likewise for ll_suffix_attn_rope_split_bf16.
 *     Semantics: HF's sliding_window_causal_mask_function over cache slots.  Key j is visible to query row r = b*S + s iff mask[r][j] != 0 and
 *     j > *pos + s - window; the mask is the one the prologues write (causal and padding) and the window is applied in the kernel, so one
 *     prologue launch serves the full and the sliding layers of a mixed model.  Everything else is the contract of the split entries: *pos is
 *     read on the device; the new rows are rotated in the launch and no workgroup reads slots *pos .. *pos+S-1 from the cache; each new row is
 *     stored by exactly one workgroup, bit for bit the row the entry points above store (a row is stored whether or not a window sees it); no
 *     atomics, fixed summation orders; a row without a visible key gives exact zeros; masked slots and slots below the window may hold
 *     anything (NaN); q_norm_w / k_norm_w as above.
 *     Geometry, a function of (B, S, nh, nkv, maxlen, D, window) only, so a captured graph replays it at every position:
 *       1. partial: nrw = min(ceil(maxlen/512), ceil((window + S - 2)/512) + 1) ranges per (head group, row) instead of ceil(maxlen/512).
 *          Workgroup x takes the ABSOLUTE range first + x, first = max(0, *pos - window + 1) / 512 computed on the device: ranges stay aligned to
 *          multiples of 512 slots.  The S windows of a call span at most window + S - 1 consecutive slots, which touch at most nrw such ranges.
 *          A range index past the end of the cache writes the empty partial (-inf, 0); mask bytes below the window are not read.
 *       2. combine: over the nrw ranges, with the operands and the order the split combine has over all ranges of the cache.
 *     Hence the output is bit for bit that of the split entry called with the window cut out of its mask, and with window >= *pos + S that of
 *     the split entry on the same mask.
 *     Bounds: 1 <= window (any int: a window the cache cannot fill costs the split entries' geometry); D, nh, nkv, B, S, maxlen, ld_qkv and the
 *     alignment as for the split entries; workspace_bytes >= ll_attn_win_workspace_bytes.  Beyond them LL_EINVAL (ll_attn_win_workspace_bytes:
 *     -1) and nothing is launched.
 * ll_attn_win_workspace_bytes : bytes of the workspace for these sizes (decode: S = 1): B*S*nh*nrw*(D+2) f32; its layout is private.  Calls on
 *     one stream may share one workspace. */
int64_t ll_attn_win_workspace_bytes(int B, int S, int nh, int nkv, int maxlen, int D, int window);
int ll_decode_attn_rope_win_bf16(const void *qkv, int64_t ld_qkv, const void *cos, const void *sin, int64_t cs_stride, void *Kc, void *Vc,
                                 const int64_t *pos, const void *mask, int64_t mask_stride, void *out, int B, int nh, int nkv, int maxlen,
                                 int D, float scale, const void *q_norm_w, const void *k_norm_w, float eps, int window, void *workspace,
                                 int64_t workspace_bytes, void *stream);
int ll_suffix_attn_rope_win_bf16(const void *qkv, int64_t ld_qkv, const void *cos, const void *sin, void *Kc, void *Vc, const int64_t *pos,
                                 const void *mask, void *out, int B, int S, int nh, int nkv, int maxlen, int D, float scale,
                                 const void *q_norm_w, const void *k_norm_w, float eps, int window, void *workspace, int64_t workspace_bytes,
                                 void *stream);
/* ---- the microscaled FP8 (OCP MXFP8) KV cache: a static cache of D + D/32 bytes per row instead of 2 D ------------------------------------
 * Storage, per cache layer four contiguous uint8 tensors: K codes and V codes [B,nkv,maxlen,D] (FP8 E4M3, OCP e4m3fn) and K scales and
 *     V scales [B,nkv,maxlen,D/32] (E8M0: the byte e + 127 of the scale 2^e shared by 32 consecutive elements of head_dim).  The stored row of a
 *     slot is the MX rounding (the quantiser of ll_wq_quantize_bf16 at 8 bits, bit for bit: amax of the block on the bf16 values, the smallest
 *     e with amax * 2^-e <= 448 clamped to [-117, 119], elements rounded to nearest, ties to even) of the bf16 row that the bf16 entry points
 *     above store: K behind the optional head RMSNorm and the rotation, V as it leaves q|k|v.  code * 2^e is exactly a bf16 number.
 *     D in {64,128}; the code tensors 8-byte aligned.
 * ll_kv8_store_bf16 : ll_kv_append_bf16 for such a cache: quantise the S rows of k_new / v_new [B,nkv,S,D] (element strides of dims 0..2,
 *     any S >= 1) into slots *pos .. *pos+S-1; rows past the last slot are dropped.
 * ll_kv8_load_bf16  : dequantise slots [0, min(maxlen, *pos + extra)) of a layer into bf16 K / V [B,nkv,maxlen,D] (16-byte aligned; the other
 *     slots are left as they are); *pos is read on the device, extra >= 0.  Exact.
 * ll_decode_attn_rope_kv8 / ll_suffix_attn_rope_kv8 : ll_decode_attn_rope_split_bf16 / ll_suffix_attn_rope_split_bf16 on such a cache, for
 *     every maxlen in 1..131072: the same arguments with the four cache tensors in place of Kc / Vc, the same two launches (partial per range
 *     of 512 keys, combine), the same workspace (ll_attn_split_workspace_bytes), bounds, masking rules and fixed summation orders; LL_EINVAL
 *     beyond the bounds, nothing launched.  Codes are expanded to f32 exactly; dots and sums are f32.  The new rows are rotated, rounded to
 *     bf16 and quantised by the workgroups whose range holds them, which attend to the DEQUANTISED row -- the result is attention over what
 *     the cache holds, at this step as at every later one; the codes and scale bytes of a slot are stored by exactly one workgroup and are
 *     bit for bit the MX rounding of the row ll_decode_attn_rope_split_bf16 stores from the same inputs.  Masked slots may hold anything (the
 *     NaN code 0x7f, the scale byte 0xff). */
int ll_kv8_store_bf16(void *Kq, void *Ks, void *Vq, void *Vs, const void *k_new, const void *v_new, const int64_t *pos, int B, int nkv, int S,
                      int maxlen, int D, const int64_t *kstr, const int64_t *vstr, void *stream);
int ll_kv8_load_bf16(const void *Kq, const void *Ks, const void *Vq, const void *Vs, void *K, void *V, const int64_t *pos, int extra, int B,
                     int nkv, int maxlen, int D, void *stream);
int ll_decode_attn_rope_kv8(const void *qkv, int64_t ld_qkv, const void *cos, const void *sin, int64_t cs_stride, void *Kq, void *Ks, void *Vq,
                            void *Vs, const int64_t *pos, const void *mask, int64_t mask_stride, void *out, int B, int nh, int nkv, int maxlen,
                            int D, float scale, const void *q_norm_w, const void *k_norm_w, float eps, void *workspace,
                            int64_t workspace_bytes, void *stream);
int ll_suffix_attn_rope_kv8(const void *qkv, int64_t ld_qkv, const void *cos, const void *sin, void *Kq, void *Ks, void *Vq, void *Vs,
                            const int64_t *pos, const void *mask, void *out, int B, int S, int nh, int nkv, int maxlen, int D, float scale,
                            const void *q_norm_w, const void *k_norm_w, float eps, void *workspace, int64_t workspace_bytes, void *stream);
/* ll_decode_prologue_dyn / ll_suffix_prologue_dyn : the two prologues for dynamic NTK rope (transformers dynamic_rope_update) without its
 *     host read of the position ids.  With L = max(position_ids of the call) + 1, read on the device by every workgroup, the frequencies are
 *     inv_freq0 [D/2] (the module's constructed original_inv_freq) while L <= max_pos (= config.max_position_embeddings) and row
 *     L - max_pos - 1 of table [table_rows, D/2] f32 beyond: row j = ROPE_INIT_FUNCTIONS["dynamic"](config, seq_len = max_pos + 1 + j).
 *     Everything else is ll_decode_prologue / ll_suffix_prologue, bit for bit.  table_rows >= maxlen - max_pos is required (LL_EINVAL
 *     otherwise: the table must cover every length the cache can reach); table may be NULL when maxlen <= max_pos.  The scaled types whose
 *     frequencies are fixed at construction (linear, llama3, yarn) need no entry point of their own: they are ll_decode_prologue with
 *     the module's inv_freq and attention_scaling. */
int ll_decode_prologue_dyn(const int64_t *position_ids, const float *inv_freq0, const float *table, int max_pos, int table_rows,
                           float attention_scaling, const int64_t *mask2d, int64_t mask_stride, const int64_t *pos, void *cos, void *sin,
                           void *mask_out, int B, int D, int maxlen, void *stream);
int ll_suffix_prologue_dyn(const int64_t *position_ids, const float *inv_freq0, const float *table, int max_pos, int table_rows,
                           float attention_scaling, const int64_t *mask2d, int64_t mask_stride, const int64_t *pos, void *cos, void *sin,
                           void *mask_out, int B, int S, int D, int maxlen, void *stream);

/* ll_linear_rows16_bf16 : out[M,N] = epilogue(x[M,K] . W^T + bias), M in 1..16, K % 32 == 0, bf16 operands, f32 accumulation on MFMA:
 *     the nn.Linear of a batched decode step (5..16 sequences: lock-step A* searches, several prompts per GPU) as a weight
 *     stream -- every wave streams its own 16 weight rows in line-contiguous segments through a private LDS image, no barrier in
 *     the main loop.  Arguments as ll_gemv_fused_bf16: norm_w != NULL = RMSNorm prologue (x is multiplied by the norm weight while it
 *     is staged and rsqrt(mean(x^2) + eps) of the row scales the accumulator: Qwen2RMSNorm + nn.Linear up to the place of one bf16
 *     rounding); epilogues LL_GEMV_PLAIN / LL_GEMV_RESIDUAL / LL_GEMV_SILU_MUL (W has 2N rows for SILU_MUL); replaces nn.Linear.forward (+ the residual add / act_fn(gate)*up of Qwen2DecoderLayer / Qwen2MLP.forward,
 *     transformers modeling_qwen2.py) under the reference's language_model.generate (modeling_llamole.py:599, :849).
 * (geometry tuning and the timing utility: include/llamole_hip_tuning.h) */
int ll_linear_rows16_bf16(const void *x, int ldx, const void *W, int ldw, const float *bias, const void *norm_w, float eps,
                          const void *residual, int ldr, void *out, int ldc, int M, int N, int K, int epi, void *stream);

/* ll_linear_rows64_bf16 : the same Linear for up to 64 token rows (17..64 sequences per GPU decoded together: the reference hands
 *     language_model.generate whatever per_device_eval_batch_size the DataLoader yields, eval/workflow.py:89-91,110-124,
 *     modeling_llamole.py:599-603; BASELINE configs[3] is 64 prompts).  Wp is a copy of the [N, K] weight ([2N, K] gate rows then up rows
 *     for LL_GEMV_SILU_MUL, N % 16 == 0) in MFMA operand order made ONCE by ll_rows64_pack_bf16 into ll_rows64_packed_elems(rows, K)
 *     bf16 elements (rows padded to a multiple of 16): weight fragments go from HBM straight into operand registers, x through an LDS
 *     ring; a persistent workgroup owns 64 weight rows x all token rows at a time, so weights are read once per launch and x once per
 *     workgroup.  K % 32 == 0.  Epilogues as ll_gemv_fused_bf16.  Matrices with few row groups (o_proj, down_proj) also split K over
 *     workgroups when `workspace` holds ll_linear_rows64_workspace_bytes(M, N) bytes of device scratch (f32 partial slabs, summed in
 *     slice order by a second launch on the same stream: deterministic); workspace = NULL keeps one launch.
 *     The RMSNorm between two Linears of a decoder layer (Qwen2RMSNorm / LlamaRMSNorm, transformers modeling_qwen2.py) is split over
 *     the two calls, so that no normalisation arithmetic sits in a GEMM's main loop:
 *       producer (plain / residual epilogue, needs the workspace): next_norm_w != NULL -> the second launch also writes
 *           scaled_out[M, N] (row stride ldn) = bf16(out * next_norm_w) and ssq_out[M, ll_rows64_ssq_chunks(N)] = per-1024-column sums
 *           of out^2;
 *       consumer: row_ssq != NULL -> x is such a scaled_out and the accumulator of token row m is multiplied by
 *           rsqrt(sum(row_ssq[m, 0..ssq_chunks)) / K + eps) before bias / epilogue (the ll_linear_rows16_bf16 form of the prologue).
 *     ll_rows64_prenorm_bf16 : scaled_out / ssq_out of a given x[M, N] alone (the embedding rows ahead of the first layer). */
int64_t ll_rows64_packed_elems(int N, int K);
int ll_rows64_pack_bf16(const void *W, int ldw, int N, int K, void *packed, void *stream);
int ll_linear_rows64_bf16(const void *x, int ldx, const void *Wp, const float *bias, const void *residual, int ldr, void *out, int ldc, int M,
                          int N, int K, int epi, const float *row_ssq, int ssq_chunks, float eps, const void *next_norm_w, void *scaled_out,
                          int ldn, float *ssq_out, void *workspace, int64_t workspace_bytes, void *stream);
int64_t ll_linear_rows64_workspace_bytes(int M, int N);
int ll_rows64_ssq_chunks(int N);
int ll_rows64_prenorm_bf16(const void *x, int ldx, const void *norm_w, void *scaled_out, int ldn, float *ssq_out, int M, int N, void *stream);

/* ---- the scaled residual epilogue and the scaled embedding (Granite layout: transformers models/granite/modeling_granite.py) -------------
 * GraniteDecoderLayer.forward adds both of its sub-blocks to the residual stream as
 *         hidden_states = residual + hidden_states * self.residual_multiplier
 * on bf16 tensors with a Python float: the product is taken in f32 with the multiplier rounded to f32 and rounded to bf16, then the sum is.
 * With the Linear's own rounding that is three roundings, and the epilogue restates them:
 *     LL_GEMV_RESIDUAL_SCALED :  bf16( residual + bf16( bf16(acc + bias) * (float)residual_scale ) )
 * residual_scale must be finite and non-zero (LL_EINVAL otherwise, nothing is launched); residual_scale == 1 gives the bits of
 * LL_GEMV_RESIDUAL.  The epilogue is not a value of `epi`: it has entry points of its own, one per Linear family, and the entries above keep
 * their signatures, their kernels and their arithmetic.  None takes an RMSNorm prologue (o_proj and down_proj have none):
 *   ll_gemv_fused_rs_bf16    ll_gemv_fused_bf16 at LL_GEMV_RESIDUAL with norm_w = NULL: M in 1..4, the same FMA order, the same choice between
 *                            the generic kernel and the one that stages x in LDS.
 *   ll_linear_rows16_rs_bf16 ll_linear_rows16_bf16 at LL_GEMV_RESIDUAL with norm_w = NULL: M in 1..16, K % 32 == 0, the same geometry.
 *   ll_linear_rows64_rs_bf16 ll_linear_rows64_bf16 at LL_GEMV_RESIDUAL: M in 1..64 on a packed weight, row_ssq / next_norm_w / workspace as
 *                            there.  One launch without a workspace; with one, the slab sum applies bias, scale and residual, and
 *                            scaled_out / ssq_out are made from the rounded scaled-residual row, as the next layer reads it.
 * ll_embed_rows_bf16 : GraniteModel.forward's `inputs_embeds * self.embedding_multiplier` with the gather in front of it, one launch:
 *     out[m, 0..H) = bf16( table[ids[m], 0..H) * (float)scale ) for ids [M] int64, table [V, H] bf16 (row stride ldt), out [M, H] (row stride
 *     ldo); f32 product, ONE rounding.  H, ldt, ldo multiples of 8, table and out 16-byte aligned, 1 <= M <= 65535, scale finite and
 *     non-zero (LL_EINVAL otherwise).  An id outside [0, V) is not an error: nothing is read for it and its row is written as zeros. */
int ll_gemv_fused_rs_bf16(const void *x, int ldx, const void *W, int ldw, const float *bias, const void *residual, int ldr, void *out, int ldc,
                          int M, int N, int K, float residual_scale, void *stream);
int ll_linear_rows16_rs_bf16(const void *x, int ldx, const void *W, int ldw, const float *bias, const void *residual, int ldr, void *out,
                             int ldc, int M, int N, int K, float residual_scale, void *stream);
int ll_linear_rows64_rs_bf16(const void *x, int ldx, const void *Wp, const float *bias, const void *residual, int ldr, void *out, int ldc, int M,
                             int N, int K, const float *row_ssq, int ssq_chunks, float eps, const void *next_norm_w, void *scaled_out, int ldn,
                             float *ssq_out, void *workspace, int64_t workspace_bytes, float residual_scale, void *stream);
int ll_embed_rows_bf16(const int64_t *ids, const void *table, int64_t ldt, void *out, int64_t ldo, int M, int V, int H, float scale,
                       void *stream);

/* ll_sample_token_bf16 : one decode-loop sampling step per row in ONE launch -- HF TemperatureLogitsWarper + TopPLogitsWarper
 *     + softmax + multinomial (transformers generation/logits_process.py, generation/utils.py _sample; the reference reaches
 *     them through language_model.generate(do_sample, temperature, top_p), modeling_llamole.py:599/:849) and the loop's
 *     bookkeeping.  logits bf16 [B,V] (row stride ld, V % 8 == 0, V <= 163840); inv_temp = 1/temperature; greedy != 0
 *     = argmax (lowest index on ties).  A value is kept iff the probability mass strictly above it is < top_p; ties with
 *     the boundary value are all kept.  Randomness: Philox4x32-10 keyed by *seed (device int64), counter (step[b], b).
 *     Per row b: t = step[b]; token = done[b] ? pad : sampled; out_tokens[b*ld_out + t] = tok[b] = token;
 *     done[b] |= token in eos[0..n_eos); step[b] = t+1; if advance: posid[b] += 1, pos[0] += 1 (either may be NULL).
 *     dbg (optional, [B,4] uint64): Z, kept mass (2^-40 fixed point), boundary key, sampled key -- parity taps. */
int ll_sample_token_bf16(const void *logits, int64_t ld, int B, int V, float inv_temp, float top_p, int greedy,
                         const int64_t *seed, const int64_t *eos, int n_eos, int64_t pad, void *done, int64_t *tok,
                         int64_t *out_tokens, int64_t ld_out, int max_new, int64_t *step, int64_t *posid, int64_t *pos,
                         int advance, uint64_t *dbg, void *stream);
/* ... with HF's TopKLogitsWarper ahead of the nucleus (the reference samples with GeneratingArguments' default top_k = 50,
 * src/hparams/generating_args.py:39-42): only the top_k highest logits survive (ties with the k-th are kept, as HF's
 * `logits < kth` test does) and top_p is applied to their renormalised distribution.  top_k <= 0 = off. */
int ll_sample_token_topk_bf16(const void *logits, int64_t ld, int B, int V, float inv_temp, float top_p, int top_k, int greedy,
                              const int64_t *seed, const int64_t *eos, int n_eos, int64_t pad, void *done, int64_t *tok,
                              int64_t *out_tokens, int64_t ld_out, int max_new, int64_t *step, int64_t *posid, int64_t *pos,
                              int advance, uint64_t *dbg, void *stream);
/* ll_sample_token_topk_ws_bf16 : the same with a workspace (ll_sample_workspace_bytes(B) bytes, 16-byte aligned, zero-filled ONCE by the
 *     caller, one per stream in flight).  With B <= 4 rows, 1 <= top_k <= 128, sampling and no dbg tap the work is split: a first launch of V/2048
 *     workgroups per row hands on the tokens that can be among the row's k largest, one workgroup per row then finishes on those -- the
 *     same token as without a workspace for every seed (the one-workgroup path also takes over, on the device, when a row has more than
 *     16384 candidates).  workspace NULL: ll_sample_token_topk_bf16. */
int64_t ll_sample_workspace_bytes(int B);
int ll_sample_token_topk_ws_bf16(const void *logits, int64_t ld, int B, int V, float inv_temp, float top_p, int top_k, int greedy,
                                 const int64_t *seed, const int64_t *eos, int n_eos, int64_t pad, void *done, int64_t *tok,
                                 int64_t *out_tokens, int64_t ld_out, int max_new, int64_t *step, int64_t *posid, int64_t *pos, int advance,
                                 uint64_t *dbg, void *workspace, int64_t workspace_bytes, void *stream);

/* Repetition penalty (HF RepetitionPenaltyLogitsProcessor, ahead of the warpers): a per-row set of the tokens seen so far on the device.
 * ll_seen_set_bytes(B, V, cap): bytes of the set for B rows, at most cap distinct tokens per row (a deduplicated list of ids, a bitmap
 *     of ceil(V/32) words and the sampler's scratch).
 * ll_seen_set_init : one launch; seeds row b from input_ids[b*ld .. b*ld + P) (pads included; P = 0: empty; ids outside [0, V) ignored).
 * ll_sample_token_penalty_bf16 : ll_sample_token_topk_bf16 on the penalised f32 logits -- every token of the row's set gets
 *     x < 0 ? x * penalty : x / penalty (inf / NaN sanitised as the raw logit is) before temperature, top-k, top-p, multinomial / argmax --
 *     and the emitted token (pad of a stopped row included) joins the set.  penalty > 0; penalty == 1: the set is kept but nothing is
 *     penalised (the same tokens as ll_sample_token_topk_ws_bf16 for every seed, as is an empty set). */
int64_t ll_seen_set_bytes(int B, int V, int cap);
int ll_seen_set_init(void *seen, int64_t seen_bytes, int B, int V, int cap, const int64_t *input_ids, int64_t ld, int P, void *stream);
int ll_sample_token_penalty_bf16(const void *logits, int64_t ld, int B, int V, float inv_temp, float top_p, int top_k, int greedy,
                                 const int64_t *seed, const int64_t *eos, int n_eos, int64_t pad, void *done, int64_t *tok,
                                 int64_t *out_tokens, int64_t ld_out, int max_new, int64_t *step, int64_t *posid, int64_t *pos, int advance,
                                 void *seen, int64_t seen_bytes, int cap, float penalty, void *stream);

/* Prompt-lookup speculative decoding of ONE sequence (HF generate(prompt_lookup_num_tokens = k, max_matching_ngram_size = n);
 * llamole_amd/llm_spec.py states the step in torch).  State, all on the device: the sampler's done / tok / out_tokens / step / posid / pos of
 * row 0, a history hist[0, *hist_len) of int64 tokens (capacity hist_cap: the call's input_ids row, then every emitted token) and the S = k + 1
 * static input rows of the captured forward, ids / position_ids / cache_position.
 * Drafting rule (PromptLookupCandidateGenerator.get_candidates): ngram sizes min(n, len - 1) down to 1; the leftmost earlier occurrence of
 *     the history's last ngram that has a non-empty continuation; the drafts d_1.. are the up to k tokens behind it.  ids[0] = *tok (the
 *     last emitted token), ids[i] = d_i, rows without a draft repeat *tok; position_ids[i] = *posid + i; cache_position[i] = *pos + i.
 * ll_spec_draft : one launch of one workgroup.  append != 0: *tok is first appended to the history (the token sampled from the prefill
 *     logits).  2 <= k <= 15, n >= 1, hist_cap >= 1; a full history is not appended to.
 * ll_spec_verify_bf16 : two launches, no host sync.  logits bf16 [S, V] of the rows ids[0..S) (row stride ld; 3 <= S <= 16, V % 8 == 0,
 *     V <= 163840, ld % 8 == 0, 16-byte aligned).  (1) Row i is sampled by the device code of ll_sample_token_topk_bf16 exactly as that
 *     samples row b = 0 at step value t + i, t = *step: same sanitising, temperature, top-k, top-p, Philox4x32-10 counter (t + i, 0) under
 *     *seed (greedy != 0: argmax, lowest index on ties) -> x_i (xs, [S] scratch).  (2) a = the number of leading i < k with
 *     x_i == ids[i + 1]; x_0..x_a are emitted, cut after the first token of eos[0..n_eos) (*done = 1) and at min(*max_new, out_cap) tokens
 *     in all; e = the number emitted.  out_tokens[t .. t + e) and the history receive them; *step += e, *posid += e, *pos += e,
 *     *cumulative_length = the new *pos (NULL: skipped; layer 0's counter of a fused cache), *tok = the last one emitted;
 *     stats[0] += 1 (forwards), stats[1] += e - 1 (accepted drafts).  With draft_next != 0 the second launch ends by writing the next
 *     step's ids / position_ids / cache_position by the rule above.  A call with *done set or *step >= min(*max_new, out_cap) writes
 *     nothing but xs.
 * Bounds violations: LL_EINVAL, nothing is launched, nothing is written. */
int ll_spec_draft(int64_t *hist, int hist_cap, int64_t *hist_len, const int64_t *tok, int append, int k, int n, const int64_t *pos,
                  const int64_t *posid, int64_t *ids, int64_t *position_ids, int64_t *cache_position, void *stream);
int ll_spec_verify_bf16(const void *logits, int64_t ld, int S, int V, float inv_temp, float top_p, int top_k, int greedy, const int64_t *seed,
                        const int64_t *eos, int n_eos, void *done, int64_t *tok, int64_t *out_tokens, int out_cap, const int64_t *max_new,
                        int64_t *step, int64_t *posid, int64_t *pos, int64_t *cumulative_length, int64_t *ids, int64_t *position_ids,
                        int64_t *cache_position, int64_t *hist, int hist_cap, int64_t *hist_len, int n, int draft_next, int64_t *stats,
                        int64_t *xs, void *stream);

/* Beam search of the graphed decode (HF GenerationMixin._beam_search; llamole_amd/llm_beam.py states the same step in torch and the
 * layout of its state): B items of nb beams, rows r = b * nb + j.
 * ll_beam_state_bytes(B, nb, K, T): bytes of the state (int32 / f32 segments: running scores, hypotheses, flags, parents, per-step
 *     tokens and parents of T steps, the row candidates); K = max(2, 1 + n_eos) * nb.
 * ll_beam_step_bf16 : one step in two launches, no host sync.  logits bf16 [B*nb, V] (row stride ld, V % 8 == 0, V <= 163840);
 *     2 <= nb <= 16, K <= 512, nb * K <= 4096, n_eos <= 32; early_stopping 0 = False, 1 = True, 2 = "never".  do_sample = beam sample:
 *     HF's Temperature (inv_temp = 1 / temperature), TopK and TopP warpers on the log-probs with min_tokens_to_keep = n_eos + 1
 *     (1 <= top_k, max(top_k, n_eos + 1) <= 512), then K draws without replacement (Gumbel-top-K, Philox4x32-10 keyed by *seed and
 *     counter (token, row, step)).  Writes tok[r] (the next input), the parents (state) and, with advance, posid[r] += 1 and
 *     pos[0] += 1.  A step after the global stop changes nothing.  Ties: the higher score, then the lower flat index beam * V + token.
 * ll_beam_kv_reorder_bf16 : one launch over all layers: kv_ptrs[n_tensors] (device) point at the StaticCache tensors [B*nb, nkv,
 *     maxlen, D] bf16; slots [*first, *pos) of row r take those of row par[r] (the state's parents; items whose parents are the
 *     identity move nothing), or with from_first_beam those of the item's beam 0.  first and pos are device int64 counters, read by
 *     the kernel.  In place; D % 8 == 0, nb * D <= 16384, n_tensors * B * nkv <= 65535.
 *     Beam sample keeps at most 1024 survivors per row: when more tokens tie at the top-k threshold value, the lowest-indexed ones;
 *     at the nucleus boundary the lower-indexed of equal tokens is removed first (HF's ascending sort taken stably). */
int64_t ll_beam_state_bytes(int B, int nb, int K, int T);
int ll_beam_step_bf16(const void *logits, int64_t ld, int B, int nb, int V, int K, int T, void *state, int64_t state_bytes,
                      const int64_t *eos, int n_eos, int max_new, float length_penalty, int early_stopping, int do_sample, float inv_temp,
                      int top_k, float top_p, const int64_t *seed, int64_t *tok, int64_t *posid, int64_t *pos, int advance, void *stream);
int ll_beam_kv_reorder_bf16(const int64_t *kv_ptrs, int n_tensors, int B, int nb, int nkv, int maxlen, int D, const int *par,
                            const int64_t *first, int from_first_beam, const int64_t *pos, void *stream);

/* ---- weight-only MX quantisation of the decode step (quantization_bit: 8 | 4; llamole_amd/csrc/llm_wq.hip) -----------------------
 * The Linear weights of a decoder layer are rounded once onto an OCP microscaling grid -- blocks of 32 consecutive elements along K, one
 * E8M0 scale 2^e per block (byte e + 127), FP8 E4M3 (e4m3fn, max 448) elements at 8 bits, FP4 E2M1 (0, 0.5, 1, 1.5, 2, 3, 4, 6) at 4 --
 * and decode calls of 1..16 token rows stream the packed codes (1.03125 / 0.53125 bytes per weight) instead of the bf16 matrix.
 * Quantiser (exact, reproducible; llamole_amd/llm_quant.py:mx_round is its torch restatement): amax = max |w| of the block; e = the
 * smallest integer with amax * 2^-e <= elem_max, taken from the exponent and mantissa bits of amax and clamped to [-117, 119] (8 bits) /
 * [-125, 125] (4 bits) so that every dequantised value is a normal bf16 number, e = 0 for an all-zero block; element = w * 2^-e rounded to
 * the nearest grid value, ties to even.  No element saturates.  code * 2^e is exactly a bf16 number: the dequantised matrix is an ordinary
 * bf16 weight, and every bf16 kernel run on it computes the same model as the packed-code kernels.
 * Layout of `packed` ([N, K] matrix, K % 32 == 0, ll_wq_bytes bytes, 16-byte aligned): N rows of K * bits / 8 code bytes (at 4 bits element
 * 2i in the low nibble of byte i), then N rows of K / 32 scale bytes.  It belongs to the kernels; read it through ll_wq_dequantize_bf16.
 *   ll_wq_bytes            size of the packed form (-1: bits not 4 | 8 or K not a multiple of 32).
 *   ll_wq_quantize_bf16    W [N, K] bf16 (row stride ldw) -> packed; Wdq != NULL also receives the dequantised bf16 matrix (row stride
 *                          lddq; may alias W; packed may then be NULL).  One launch, no host synchronisation.
 *   ll_wq_dequantize_bf16  packed -> W [N, K] bf16, through the hardware conversions the kernels use.
 *   ll_gemv_fused_wq       ll_gemv_fused_bf16 on a packed weight (M in 1..4; RMSNorm prologue with K <= 8192; plain /
 *                          residual / SiLU*mul epilogues with the same bf16 roundings; LL_GEMV_SILU_MUL: packed holds 2N rows, gate rows
 *                          then up rows); the M rows of x, each padded to a multiple of 1024 (8 bits) / 2048 (4 bits) elements, plus
 *                          16 M bytes must fit the 160 KB of LDS.
 *   ll_linear_rows16_wq    ll_linear_rows16_bf16 on a packed weight (M in 1..16): each wave expands the codes of its 16 weight rows to
 *                          bf16 on the way into its LDS image; same prologue and epilogues. */
int64_t ll_wq_bytes(int N, int K, int bits);
int ll_wq_quantize_bf16(const void *W, int ldw, int N, int K, int bits, void *packed, void *Wdq, int lddq, void *stream);
int ll_wq_dequantize_bf16(const void *packed, int N, int K, int bits, void *W, int ldw, void *stream);
int ll_gemv_fused_wq(const void *x, int ldx, const void *packed, int bits, const float *bias, const void *norm_w, float eps,
                     const void *residual, int ldr, void *out, int ldc, int M, int N, int K, int epi, void *stream);
int ll_linear_rows16_wq(const void *x, int ldx, const void *packed, int bits, const float *bias, const void *norm_w, float eps,
                        const void *residual, int ldr, void *out, int ldc, int M, int N, int K, int epi, void *stream);

/* ---- sparse mixture-of-experts MLP block at decode (Qwen3-MoE layout; llamole_amd/csrc/llm_moe.hip) --------------------------------
 * Replaces Qwen3MoeSparseMoeBlock.forward (transformers modeling_qwen3_moe.py: Qwen3MoeTopKRouter + Qwen3MoeExperts) + the decoder layer's
 * residual add for 1..64 token rows.  The router logits are NOT an entry point of their own: they are ll_gemv_fused_bf16 /
 * ll_linear_rows16_bf16 with W = mlp.gate.weight [E, H], the post-attention RMSNorm as prologue and the LL_GEMV_PLAIN epilogue (HF's
 * F.linear on the normalised row, rounded to bf16).  All three calls are enqueued on `stream`, read the routing on the device only (no
 * host synchronisation) and have a launch geometry that depends on (M, E, top_k, H, I) alone, so a captured graph replays them.
 * Bounds of all three: 1 <= M <= 64, E <= 256, 1 <= top_k <= min(E, 8); beyond them LL_EINVAL (ll_moe_workspace_bytes: -1), nothing is launched.
 *
 * ll_moe_workspace_bytes : bytes of the device workspace (16-byte aligned) the two calls below share for these sizes; its layout is private.
 *     A workspace sized for 64 rows serves every smaller M.
 *
 * ll_moe_route_bf16 : logits [M, E] bf16 (row stride ld elements) -> idx [M, top_k] int32 and w [M, top_k] bf16, both contiguous, in slot
 *     order (Qwen3MoeTopKRouter.forward):
 *       selection      the top_k largest logits in descending order, equal logits by the lower expert index (softmax is monotone: this is
 *                      torch.topk(softmax(logits)) wherever torch's result is determined); a NaN logit ranks below every number;
 *       probabilities  p_j = exp(l_j - max) / sum_all_i exp(l_i - max), f32;
 *       weights        w_j = p_j / sum_selected p (f32, summed in slot order) when norm_topk != 0, else p_j; ONE rounding to bf16.
 *     It also writes the grouping of the (row, slot) pairs by expert that ll_moe_experts_bf16 reads into the workspace.
 *
 * ll_moe_experts_bf16 : x [M, H] = the UN-normalised residual stream (row stride ldx), norm_w [H] / eps = the post-attention RMSNorm,
 *     idx / w / workspace = what ll_moe_route_bf16 wrote for the same (M, E, top_k) (expert ids are trusted to lie in [0, E); addresses are
 *     clamped into the operands whatever the workspace holds), Wgu [E, 2I, H] (gate rows then up rows per expert:
 *     Qwen3MoeExperts.gate_up_proj in place), Wd [E, H, I] (down_proj in place), residual [M, H] (stride ldr), out [M, H] (stride ldo;
 *     may alias residual).  For token row m and slot j with e = idx[m, j]:
 *         a_mj  = the LL_GEMV_SILU_MUL result of ll_gemv_fused_bf16 with its RMSNorm prologue on x_m and W = Wgu[e]
 *                 (the same device function: same arithmetic, same bf16 roundings)
 *         y_mj  = bf16( a_mj . Wd[e]^T )                          f32 accumulation, the dense GEMV's order
 *         z_mj  = bf16( float(w_mj) * float(y_mj) )
 *         out_m = bf16( float(residual_m) + float( bf16( sum_j z_mj ) ) )      sum in f32, slot order, ONE rounding
 *     This is HF's default experts path (grouped_mm: view(tokens, k, H).sum(dim=1)) followed by the layer's residual add.  The one
 *     deviation: HF's `eager` experts implementation accumulates the k terms in bf16 with index_add_ in expert order instead.
 *     A token row that is the only one of its expert gets bit for bit what ll_gemv_fused_bf16 gives on that expert's matrices.
 *     Three launches (gate|up, down, slot sum + residual) over min(E, M * top_k) active-expert slots: experts nobody chose cost nothing,
 *     and an expert's matrices are streamed from HBM once per launch however many rows chose it (passes of up to 4 rows).
 *     Sizes: H % 8 == 0, 8 <= H <= 8192, I % 8 == 0, 8 <= I <= 32768, strides multiples of 8, operands 16-byte aligned, eps > 0. */
int64_t ll_moe_workspace_bytes(int M, int E, int top_k, int H, int I);
int ll_moe_route_bf16(const void *logits, int ld, int M, int E, int top_k, int norm_topk, int32_t *idx, void *w, void *workspace,
                      int64_t workspace_bytes, void *stream);
int ll_moe_experts_bf16(const void *x, int ldx, const void *norm_w, float eps, const int32_t *idx, const void *w, const void *Wgu,
                        const void *Wd, const void *residual, int ldr, void *out, int ldo, int M, int E, int top_k, int H, int I,
                        void *workspace, int64_t workspace_bytes, void *stream);

/* ---- the same block in the Mixtral and the shared-expert (Qwen2-MoE) layouts ----------------------------------------------------------
 * MixtralSparseMoeBlock (transformers modeling_mixtral.py) and Qwen2MoeSparseMoeBlock (modeling_qwen2_moe.py) keep the parts above -- experts
 * as gate_up_proj [E, 2I, H] / down_proj [E, H, I], a router weight [E, H], SiLU, no biases -- and differ from the Qwen3 contract in two pieces
 * of arithmetic.  Bounds, workspace (ll_moe_workspace_bytes, unchanged), stream behaviour and launch counts are those of the calls above.
 *
 * ll_moe_route_f32 : ll_moe_route_bf16 with w [M, top_k] written as FLOAT, the f32 value itself, never rounded to bf16 (MixtralTopKRouter keeps
 *     its renormalised weights in f32; it always renormalises: pass norm_topk = 1).  Selection, tie rule, grouping and workspace layout are
 *     those of ll_moe_route_bf16.
 *
 * ll_moe_experts_ex_bf16 : ll_moe_experts_bf16 with two options; with both off (w_f32 == 0, shared == NULL) it IS that call, bit for bit.
 *   w_f32 != 0 (Mixtral): w is the float [M, top_k] of ll_moe_route_f32.  The down launch stores the unweighted y_mj where z_mj stood and
 *     the slot sum applies the weight:
 *         y_mj  = bf16( a_mj . Wd[e]^T )
 *         out_m = bf16( float(residual_m) + float( bf16( sum_j f32( w_mj * float(y_mj) ) ) ) )
 *     every product rounded to f32 on its own (no fused multiply-add), the sum in f32 in slot order, ONE rounding to bf16: HF's default
 *     experts path on f32 weights (bf16 * f32 -> f32, view(tokens, k, H).sum(dim=1), one cast).  No per-slot rounding z_mj = bf16(w y).
 *   shared != NULL (Qwen2-MoE): shared [M, H] bf16 (row stride lds elements, a multiple of 8, 16-byte aligned) holds the shared expert's
 *     output s_m = shared_expert(rmsnorm(x_m)) -- computed by the caller with the dense MLP's own kernels (ll_gemv_fused_bf16 /
 *     ll_linear_rows16_bf16 / ll_linear_rows64_bf16: gate|up with the RMSNorm prologue and the SiLU*mul epilogue, down with the plain one) --
 *     and gate[m * ldg] (bf16, any ldg >= 1: a column of a wider matrix) the logit g_m = bf16(rmsnorm(x_m) . shared_expert_gate.weight[0]).
 *     With e_m = bf16(sum_j z_mj) (or the w_f32 sum above):
 *         sig_m = bf16( 1 / (1 + exp(-float(g_m))) )                                             f32 evaluation
 *         out_m = bf16( float(residual_m) + float( bf16( float(e_m) + float( bf16( float(sig_m) * float(s_m) ) ) ) ) )
 *     i.e. F.sigmoid(shared_expert_gate(x)) * shared_expert(x) added to the experts' output, then the layer's residual add, each a bf16 tensor
 *     operation of HF's forward.
 *   Three launches, as ll_moe_experts_bf16.  A bound violated returns LL_EINVAL and launches nothing. */
int ll_moe_route_f32(const void *logits, int ld, int M, int E, int top_k, int norm_topk, int32_t *idx, float *w, void *workspace,
                     int64_t workspace_bytes, void *stream);
int ll_moe_experts_ex_bf16(const void *x, int ldx, const void *norm_w, float eps, const int32_t *idx, const void *w, int w_f32, const void *Wgu,
                           const void *Wd, const void *residual, int ldr, const void *shared, int lds, const void *gate, int ldg, void *out,
                           int ldo, int M, int E, int top_k, int H, int I, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LLAMOLE_HIP_H */
