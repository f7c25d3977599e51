/* libtrace_hip.so — C ABI of the MI355X-native TRACE inference hot path.
 *
 * The reference (gyxxyg/TRACE) is 100% Python and has no FFI of its own; its arithmetic lives in
 * transformers/torch.  This header is the boundary a maintainer binds instead (ctypes stub in INTEGRATION.md):
 * everything from the sampled frame tensor to the greedy token ids.  Each entry point cites the reference
 * interface it replaces (paths relative to the reference repo root).
 *
 * Conventions: extern "C"; every function returns 0 on success or a negative TRACE_ERR_* code, the message is
 * available from trace_last_error(); no C++ exceptions cross the ABI; pointers are raw device (or, where
 * stated, host) addresses + explicit sizes; `stream` is a hipStream_t passed as void* (0 = default stream).
 * A trace_ctx owns its weights, KV cache and workspaces (hipMalloc) and is not thread-safe; one per process/GPU.
 * All device tensors are bf16 (uint16 bit patterns) unless stated.
 */
#ifndef TRACE_HIP_H
#define TRACE_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define TRACE_ABI_VERSION 4

typedef struct trace_ctx trace_ctx;

/* Geometry: the config.json keys the reference reads (trace/model/language_model/trace_mistral.py:84-96,
 * trace/model/multimodal_encoder/clip_encoder.py:15-16, trace/model/multimodal_projector/builder.py:413-421). */
typedef struct trace_config {
    int32_t vocab_size, hidden_size, intermediate_size, num_layers, num_heads, num_kv_heads;
    int32_t time_vocab, score_vocab;
    float rms_eps, rope_theta;
    int32_t v_hidden, v_inter, v_layers_used, v_heads, v_image, v_patch;
    float v_eps;
    int32_t num_slots;
    float slot_eps, slot_rope_base;
    int32_t max_frames;      /* largest T per video                                    */
    int32_t max_ctx;         /* KV-cache length per sequence slot (prefill + new tokens) */
    int32_t max_batch;       /* KV-cache sequence slots, <= 512; one decode batch takes at most 256 of them (64 on the fp8 and w4 weight paths; the rest can be
                              * prefilled meanwhile: trace_amd.engine.TraceEngine.generate_stream) */
    int32_t max_new_tokens;  /* capacity of the on-device output id buffer               */
    int32_t projector_type;  /* 0 = spatial_slot (TRACE), 1 = stc_connector (legacy API) */
    int32_t vit_batch_frames; /* frames one trace_vit_forward call may take (ViT workspaces); 0 = max_frames.  Larger than
                               * max_frames lets a caller push the frames of several videos through the tower together (the
                               * tower is per-frame: results do not depend on the grouping) */
    int32_t llm_weights_fp8;  /* the four decoder projections per layer on the fp8 path (BASELINE config 5): e4m3 weights with a scale per output
                               * row made at load from the bf16 tensors.  1 = W8A8 everywhere: activations quantised per token row on the
                               * fly, fp8 MFMA with fp32 accumulation.  2 = W8A8 prefill GEMMs, WEIGHT-ONLY decode GEMVs (bf16 activations,
                               * weights widened to bf16 in registers, bf16 MFMA): the same weight bytes per step, half the rounding-noise
                               * variance where the tokens are chosen.  No reference counterpart; parity anchor = the bf16 path */
} trace_config;

const char* trace_last_error(void);
int trace_abi_version(void);
/* The library's 16-bit element type: 0 = bf16 (libtrace_hip.so), 1 = IEEE fp16 (libtrace_hip_f16.so: the same sources compiled with -DTRACE_F16 —
 * the reference's own inference dtype, torch.float16, trace/model/builder.py:50,127,147 / trace/eval/evaluate.py:316).  Every "bf16" in this header
 * reads "the library's element type"; the two libraries export the same symbols and may be loaded side by side (RTLD_LOCAL). */
int trace_element_type(void);

/* from_pretrained (trace/model/builder.py:113-114): create, stream tensors in by their reference state-dict
 * names (bf16; `on_device` says whether `data` is a device or host pointer), then finalize. */
int trace_ctx_create(const trace_config* cfg, int device_id, trace_ctx** out);
/* trace_ctx_create with options (trace_config is frozen at ABI version 4).  size = sizeof(trace_ctx_opts) of the caller (8), or sizeof(trace_ctx_opts_w4)
 * (12: the form below with llm_weights_w4 behind the two fields); a smaller size is TRACE_ERR_ARG.  kv_cache_fp8 = 1: the context
 * keeps its KV cache as e4m3 bytes with one fp32 scale per position and kv head (the "kv8" format, stated at the end of this header) — 264 bytes per
 * position and kv head instead of 512, i.e. about twice the sequences or context per card — plus one layer's 16-bit K / V^T of 8 slots that every prefill
 * stages through.  opts == NULL or a zero flag is trace_ctx_create.  Under kv_cache_fp8:
 *   - a prefill of whole prompts computes the bits the 16-bit-cache context computes (hidden rows, last-position row, step-0 logits): its attention runs
 *     on the 16-bit staging rows, which are quantised into the cache afterwards;
 *   - trace_llm_prefill_append first dequantises the cached rows it continues, so the new rows attend the QUANTISED past — what the decode steps see.
 *     Deterministic, but not the bits of an uncut prefill: "a row's bits do not depend on where the prompt was cut" is the 16-bit cache's promise;
 *   - every decode step appends with a launch of its own (the route trace_op_decode_route out[2] = 1 describes) and attends the e4m3 cache;
 *   - trace_kv_copy moves the e4m3 arrays (whole 32-position blocks), trace_debug_buffers answers TRACE_ERR_STATE (trace_debug_kv8_buffers).
 * TRACE_ERR_ARG, checked before any device call: kv_cache_fp8 outside {0, 1}; kv_cache_fp8 with llm_weights_fp8 != 0 (fp8 weights over an fp8 cache
 * is out of scope). */
typedef struct trace_ctx_opts { int32_t size; int32_t kv_cache_fp8; } trace_ctx_opts;
int trace_ctx_create_opts(const trace_config* cfg, int device_id, const trace_ctx_opts* opts, trace_ctx** out);
int trace_ctx_kv_cache_type(trace_ctx* ctx);            /* 0 = element type, 1 = e4m3 + scales */
/* The 12-byte form of the options: trace_ctx_create_opts reads llm_weights_w4 when the caller's size says the field is there (cast the pointer); the
 * 8-byte struct above keeps working and means llm_weights_w4 = 0.  llm_weights_w4 = 1: the context keeps the four decoder projections of every layer
 * (qkv, o, gate|up, down) in the "w4" format stated at the end of this header — 4-bit e2m1 codes with one power-of-two scale per 32 weights, 4.25 bits
 * a weight — as its ONLY copy of them, in the decode tile layout, plus one layer's worth of 16-bit row-major scratch.  Embedding, heads, norms, ViT
 * and slot pool stay 16-bit.  trace_ctx_load_tensor quantises a projection as it arrives; trace_ctx_device_bytes reports the saving.  Under w4:
 *   - every prefill (trace_llm_prefill, _pair, _multi, _append, _shared, trace_llm_score_append) dequantises a layer's four tensors into the scratch
 *     before the layer and runs the 16-bit GEMMs on it unchanged; the decode GEMVs widen the codes to bf16 in registers.  Both multiply by the same
 *     matrix W~ (every w4 value is exactly a bf16 value), and activations are never quantised: a context of 16-bit weights loaded with W~ computes
 *     the prefill's bits exactly, and the continuation promise of trace_llm_prefill_append holds as on 16-bit weights (trace_kv_copy,
 *     trace_llm_prefill_shared and trace_decode_set_shared_prefix stay available);
 *   - at most 64 sequences decode together (trace_decode_begin answers TRACE_ERR_ARG above), on the GEMV step (trace_op_decode_route_w4).
 * TRACE_ERR_ARG, checked before any device call: llm_weights_w4 outside {0, 1}; with llm_weights_fp8 != 0; with kv_cache_fp8; in the fp16 library;
 * hidden_size or intermediate_size not a multiple of 256. */
typedef struct trace_ctx_opts_w4 { int32_t size; int32_t kv_cache_fp8; int32_t llm_weights_w4; } trace_ctx_opts_w4;
int trace_ctx_llm_weights_type(trace_ctx* ctx);         /* 0 = element type, 1 / 2 = trace_config.llm_weights_fp8, 3 = w4 */
int trace_ctx_destroy(trace_ctx* ctx);
int trace_ctx_load_tensor(trace_ctx* ctx, const char* name, const void* data, int on_device, const int64_t* shape,
                          int ndim);
int trace_ctx_finalize(trace_ctx* ctx);
int64_t trace_ctx_device_bytes(trace_ctx* ctx);

/* Frame preprocessing of process_video (trace/mm_utils.py:456-462; expand2square :259-270; HF CLIPImageProcessor.preprocess of
 * transformers 4.40.1: resize shortest edge -> v_image with Pillow BICUBIC, centre crop, x/255, (x - mean)/std), on the device:
 * frames_u8 [T,H,W,3] uint8 RGB (device) -> out [T,3,v_image,v_image] (out_dtype 0 = bf16, 1 = fp32; device).
 * pad_to_square = the drivers' aspect_ratio == 'pad' (background int(mean*255)).  image_mean / image_std: 3 host floats.
 * The resize reproduces Pillow's 8-bit two-pass fixed-point resampler bit for bit; fp32 output equals the reference's
 * FloatTensor exactly. */
int trace_preprocess_frames(trace_ctx* ctx, const void* frames_u8, int T, int H, int W, int pad_to_square,
                            const float* image_mean, const float* image_std, void* out, int out_dtype, void* stream);

/* CLIPVisionTower.forward + feature_select (trace/model/multimodal_encoder/clip_encoder.py:31-53):
 * frames [T,3,S,S] (dtype 0 = bf16, 1 = fp32, device) -> features [T, patches, v_hidden] bf16 = hidden state
 * after encoder layer v_layers_used, CLS dropped.  feats_out may be NULL (kept internally for trace_slot_pool). */
int trace_vit_forward(trace_ctx* ctx, const void* frames, int frames_dtype, int T, void* feats_out, void* stream);

/* SpatialSlotPool.forward (trace/model/multimodal_projector/builder.py:427-467): feats (NULL = the internal
 * buffer of the last trace_vit_forward) -> slots_out [T, num_slots, hidden]; slots_out may be NULL. */
int trace_slot_pool(trace_ctx* ctx, const void* feats, int T, void* slots_out, void* stream);

/* STCConnector.forward (trace/model/multimodal_projector/builder.py:208-249), legacy trace.infer() path only
 * (projector_type = 1): feats [T, patches, v_hidden] (NULL = internal buffer of the last trace_vit_forward) ->
 * out [(T/2+1) * (g/2+1)^2, hidden] (may be NULL; the result also becomes the internal video rows for
 * trace_splice_embeds).  *rows_out receives the row count.  Parity of this connector is unpinned (timm absent). */
int trace_stc_connector(trace_ctx* ctx, const void* feats, int T, void* out, int* rows_out, void* stream);

/* encode_images_or_videos (trace/model/trace_arch.py:218-266): ViT + slot pool + per-frame time-token embedding;
 * time_ids is HOST int32 [T, 6] (TimeTower.encode(t)[:-1]).  Result [T*(slots+6), hidden] stays internal;
 * video_out (device, may be NULL) receives a copy. */
int trace_encode_video(trace_ctx* ctx, const void* frames, int frames_dtype, int T, const int32_t* time_ids,
                       void* video_out, void* stream);

/* The same from ViT features computed earlier (trace_vit_forward with feats_out, possibly in a call that carried the frames
 * of several videos, see vit_batch_frames): feats [T, patches, v_hidden] bf16 (device) -> slot pool + time-token rows. */
int trace_encode_features(trace_ctx* ctx, const void* feats, int T, const int32_t* time_ids, void* video_out, void* stream);

/* prepare_inputs_labels_for_multimodal, prefill branch (trace/model/trace_arch.py:377-456): HOST ids with the
 * modal placeholders (-201 video, -203 time, -204 score, -205 sync); the single video placeholder expands to
 * the rows of the last trace_encode_video.  time_rows/score_rows: HOST tower row ids consumed in order by the
 * -203/-204 placeholders (may be NULL).  Writes the spliced embeddings internally, returns their length in
 * *L_out; embeds_out (device [L,hidden], may be NULL) receives a copy. */
int trace_splice_embeds(trace_ctx* ctx, const int32_t* ids, int n_ids, const int32_t* time_rows, int n_time,
                        const int32_t* score_rows, int n_score, int* L_out, void* embeds_out, void* stream);

/* TraceMistralForCausalLM.forward, prefill (trace/model/language_model/trace_mistral.py:114-264): runs the L
 * spliced rows (embeds == NULL: internal buffer) through the decoder into KV slot `slot`.  hidden_out (device
 * [L,hidden] bf16, may be NULL) receives the final-norm hidden states (tests). */
int trace_llm_prefill(trace_ctx* ctx, int slot, const void* embeds, int L, void* hidden_out, void* stream);
/* Two prompts of EQUAL spliced length prefilled in one pass (GEMM M = 2L fills the MFMA tile grid in whole rounds): embeds0 / embeds1
 * [L, hidden] bf16 device (the embeds_out of two trace_splice_embeds calls) -> KV slots slot0 and slot0 + 1.  Same results as two
 * trace_llm_prefill calls. */
int trace_llm_prefill_pair(trace_ctx* ctx, int slot0, const void* embeds0, const void* embeds1, int L, void* stream);
/* The same for n <= 8 prompts of equal length while n * L <= max(4 * max_ctx, min(8192, 8 * max_ctx)) rows (the prefill workspaces; more -> TRACE_ERR_ARG):
 * embeds = HOST array of n device pointers ([L, hidden] bf16 each) -> KV slots slot0 .. slot0 + n - 1.  M = 4 L = 7868 at the C2 shape fills the 256x256
 * tile grid of every projection in whole rounds; at the C4 shape (L = 1086) seven prompts do (30 row panels: the o / down grid in 1.9 rounds where four
 * prompts' 17 panels need 2 rounds for 1.06 of work).  Results per prompt do not depend on n. */
int trace_llm_prefill_multi(trace_ctx* ctx, int slot0, const void* const* embeds, int n, int L, void* stream);

/* One video, several questions (trace/eval/videomme/evaluate.py:349-386 calls model.generate once per entry of qa_list with the same frame tensor, the
 * same timestamps and a prompt identical up to and including <video>; trace/eval/mvbench and any multi-turn use of one video do the same): the rows
 * through <video> are prefilled once and kept, each question prefills only the rows after them.
 * n <= 8 slots slot0 .. slot0+n-1, each holding at least `past` rows: run L new rows per slot at positions past .. past+L-1 attending rows
 * 0 .. past+L-1; rows >= past that the slot held before are discarded.  embeds: HOST array of n device pointers [L, hidden]; NULL with n == 1 = the
 * internal embedding buffer (the last trace_embed_rows / trace_splice_embeds).  hidden_out (n == 1 only, may be NULL): [L, hidden] final-norm rows.
 * past == 0 is trace_llm_prefill_multi.  A row's results are bit-identical to the same row of one trace_llm_prefill over all past + L rows, wherever
 * the cut is, on the bf16, fp16 and fp8 paths.  TRACE_ERR_STATE: past above the rows a slot holds; TRACE_ERR_ARG: past < 0, past + L > max_ctx, n x L
 * above the prefill workspace (see trace_llm_prefill_multi), a slot out of range — all before any launch. */
int trace_llm_prefill_append(trace_ctx* ctx, int slot0, int n, int past, const void* const* embeds, int L, void* hidden_out, void* stream);
/* rows [0, rows) of every layer's K and V^T from src_slot to n other slots (HOST dst_slots); their length becomes `rows` (the V^T side may copy up to 7
 * positions more: finite values that a later append overwrites and the attention masks).  rows == the source's length: the copies can be decoded from as
 * the source can.  TRACE_ERR_STATE: rows above the source's length; TRACE_ERR_ARG: a slot out of range, src_slot among the destinations. */
int trace_kv_copy(trace_ctx* ctx, int src_slot, const int32_t* dst_slots, int n, int rows, void* stream);
/* A batch whose prompts all begin with the same `past` rows (the ids before <video>, one question for every video): prefill those rows ONCE into one
 * slot (trace_llm_prefill), then call this for every run of n <= 8 equal-length prompts: rows [0, past) of src_slot are copied to the run's slots
 * (trace_kv_copy's launches; src_slot may be one of them and may by then hold more rows) and the n prompts continue with their own L rows each
 * (trace_llm_prefill_append(past)'s body, no hidden_out) — one call per run.  By the promise above the slots end up with the bits n whole prefills would
 * have left.  TRACE_ERR_STATE: an e4m3 KV cache or fp8 weights (a continuation is not bit-identical there), past above the source's length; otherwise
 * trace_llm_prefill_append's argument rules, all checked before the first launch. */
int trace_llm_prefill_shared(trace_ctx* ctx, int src_slot, int slot0, int n, int past, const void* const* embeds, int L, void* stream);
/* trace_splice_embeds for rows that hold no <video> (the part of a prompt after the placeholder, trace/model/trace_arch.py:410-427 for those rows):
 * token / <sync> / <time> / <score> ids -> [n_ids, hidden] (internal buffer; embeds_out may be NULL).  A video placeholder among the ids is
 * TRACE_ERR_ARG; trace_splice_embeds itself keeps its "only have one video" rule. */
int trace_embed_rows(trace_ctx* ctx, const int32_t* ids, int n_ids, const int32_t* time_rows, int n_time, const int32_t* score_rows, int n_score,
                     void* embeds_out, void* stream);

/* The head stage of forward() for EVERY position (trace_mistral.py:190-252: lm_head | sync_head | time_head | score_head, fp32,
 * everything outside head `head`'s id range set to -inf): hidden [R, hidden] bf16 device = the hidden_out of trace_llm_prefill ->
 * logits_out [R, V+1+Tv+Sv] fp32 device.  The decode loop needs the last row only and gets it from trace_decode_begin / _steps. */
int trace_llm_head_logits(trace_ctx* ctx, const void* hidden, int R, int head, float* logits_out, void* stream);

/* Scoring GIVEN tokens: how likely is this continuation?  (Multiple-choice scoring of the per-question drivers, trace/eval/videomme/evaluate.py; ranking
 * candidate captions or moments; teacher-forced log-likelihood of a [time | score | caption] stream.)  trace_decode_begin(forced = ...) with
 * log-probabilities records the model's OWN choice at every step; these entry points score the ids that are fed.
 * A continuation is a list of global vocabulary ids c[0 .. n) over [text | <sync> | time | score] and the head h0 active for c[0] (callers pass 1, as
 * generate does).  The head of position i follows the switch rule of the decode step applied to the FED ids:
 *     head[0] = h0,   head[i + 1] = c[i] == V ? 1 : c[i] == V + 1 ? 2 : c[i] == V + Tv + 1 ? 0 : head[i]
 * and its log-probability is
 *     logprob[i] = (x[c[i]] - M) - log S,   M = max x,   S = sum exp(x - M)
 * over the raw fp32 logits x of head[i]'s id range [lo, hi), taken from the final-norm hidden row that PRECEDES c[i]: the last prompt row for c[0], the
 * row fed with the embedding of c[i - 1] otherwise (the decode branch's embedding rule = trace_embed_rows with the matching placeholders).  An id outside
 * [lo, hi) gives -inf; id -1 means "ignore" (padding) and gives 0.0; a continuation's score is the plain sum of its entries.
 * The sums, so that a float32 restatement (trace_amd/sampling.py score_logprob_ref) gives the device's bits from the same fp32 logits: the head's range is
 * cut into column tiles [j CT, (j + 1) CT) on ABSOLUTE ids, CT = trace_op_score_tile() = 128, clipped to [lo, hi).  Per tile: m_j = max x,
 * s_j = h0 + h1 where h0 / h1 sum exp(x - m_j) over the tile's lower / upper 64 columns, each sequentially in ascending id order from 0.  Then
 * M = max_j m_j, S = sum_j s_j * exp(m_j - M) sequentially in ascending j from 0 (S >= 1), exp / log = csrc/sample.h sample_exp / sample_log, no FMA
 * contraction.  The logits themselves are never stored: text rows run a 16-bit MFMA GEMM (K = hidden, fp32 accumulation) against the V + 1 rows of the
 * lm | sync block whose epilogue leaves (m_j, s_j, x_target) per row and tile; time / score rows (Tv, Sv <= 128) are dot products in the merge kernel.
 *
 * trace_op_score_rows: loose rows.  hidden [R][ld], W [V + 1 + Tv + Sv][ldw] head rows in global vocabulary order, both the library's element type,
 *     row length K (K % 64 == 0, ld / ldw >= K and % 8 == 0); heads / ids int32 [R] DEVICE; ws: trace_op_score_ws_bytes(R, V, Tv, Sv) bytes of device
 *     scratch; out fp32 [R] device.  R <= 65536.  Heads outside 0..2 are read as 2, ids are not range-checked beyond "outside the head" (device arrays).
 * trace_llm_score_rows: the same over the context's head matrix; hidden [R][hidden] = final-norm rows (the hidden_out of a prefill), R at most the
 *     prefill workspace's rows; the scratch is allocated on first use.
 * trace_llm_score_append: the body of trace_llm_prefill_append for n <= 8 slots followed by the score of all n x L final-norm rows: row (b, i) is
 *     scored against ids[b * L + i] under heads[b * L + i].  heads / ids are HOST int32 [n * L], out is a HOST float [n * L]; the call synchronises the
 *     stream.  Afterwards the slots hold past + L rows, as after trace_llm_prefill_append.  Every argument error of trace_llm_prefill_append applies
 *     (there is no hidden_out here); in addition TRACE_ERR_ARG for a head outside 0..2 and an id < -1 or >= V + 1 + Tv + Sv — all before any launch.
 *     Works on the fp8-weight paths and under kv_cache_fp8 (where, as for trace_llm_prefill_append, the new rows attend the QUANTISED past). */
int trace_op_score_tile(void);
int64_t trace_op_score_ws_bytes(int R, int V, int Tv, int Sv);
int trace_op_score_rows(const void* hidden, int ld, const void* W, int ldw, int K, int R, const int32_t* heads, const int32_t* ids, int V, int Tv, int Sv,
                        void* ws, float* out, void* stream);
int trace_llm_score_rows(trace_ctx* ctx, const void* hidden, int R, const int32_t* heads, const int32_t* ids, float* out, void* stream);
int trace_llm_score_append(trace_ctx* ctx, int slot0, int n, int past, const void* const* embeds, int L, const int32_t* heads, const int32_t* ids,
                           float* out, void* stream);

/* generate() = greedy loop with head switching (trace_mistral.py:268-347 + HF greedy search).
 * begin: sequences = the given KV slots (each prefilled); heads[b] in {0 text,1 time,2 score} (callers pass [1]);
 *        computes token 0 from the prefill hidden state.  forced: HOST [B, max_new] teacher-forcing ids or NULL.
 *        eos < 0 disables the stop.  logits_out (device fp32 [B, V+1+Tv+Sv], may be NULL) = masked logits of step 0.
 * steps: runs n more decode steps entirely on device (use_graph: hipGraph replay; logits_out only with n == 1).  At most
 *        max_new - 1 steps in total after one begin (every step appends a KV row; TRACE_ERR_STATE beyond).
 * read : synchronises and copies ids [B, max_new] / lengths [B] / current heads [B] to HOST buffers. */
int trace_decode_begin(trace_ctx* ctx, const int32_t* slots, int B, const int32_t* heads, int max_new, int eos,
                       const int32_t* forced, float* logits_out, void* stream);
int trace_decode_steps(trace_ctx* ctx, int n, int use_graph, float* logits_out, void* stream);
int trace_decode_read(trace_ctx* ctx, int32_t* out_ids, int32_t* out_len, int32_t* heads, void* stream);
/* Retire rows of the running batch.  Shrink the batch begun by trace_decode_begin to n_keep rows: new row i is former row keep[i].  keep (HOST) is
 * strictly increasing, within [0, B).  Everything a step reads or writes per row moves with the row: slot, position, head, done flag, length, the
 * rows of recorded ids, forced ids and (when armed) log-probabilities, and the embedding the next step consumes.  The Philox row index of a row
 * stays the index it had at trace_decode_begin, so a sampled row draws what it would have drawn in the full batch.  Results of dropped rows must
 * have been read (trace_decode_read, trace_decode_read_logprobs) before the call; afterwards those calls return n_keep rows.  The step counter, the
 * steps taken and max_new stay as they are; a shared prefix stays in force while two rows or more remain.  The next trace_decode_steps runs the step
 * of the new batch size (a graph of its own, captured the first time that size is seen): on real weights its rounding is that batch size's, as it
 * is for a batch begun at that size.  n_keep == B is a no-op that launches nothing.  Returns after the stream has run the gather.
 * TRACE_ERR_STATE: no batch begun; host-select mode.  TRACE_ERR_ARG: n_keep < 1 or > B; an index outside [0, B); a list that is not strictly
 * increasing.  After an error the batch is as it was. */
int trace_decode_retire(trace_ctx* ctx, const int32_t* keep, int n_keep, void* stream);
/* Admit rows into the running batch.  Append n prefilled sequences (KV slots `slots`, HOST) behind the B rows of the batch begun by
 * trace_decode_begin: the batch becomes B + n rows, the new ones last (retire first, then admit: rows never land in holes).  For the new rows the call
 * does what trace_decode_begin does for a batch (position = the slot's prefill length, heads[i], done = 0, length 0, zeroed ids and, when armed,
 * log-probabilities, forced ids = forced [n][max_new] HOST or none) and then computes THEIR token 0 from the prefill hidden state, on those rows alone:
 * the rows already running, and the step counter they share, do not move.  A row keeps a step count of its own from there: its recorded ids, length,
 * forced ids, log-probabilities, max_new, min_new_tokens, begin_suppress_tokens, stop match and Philox counter are those of a row begun at its step 0.
 * row_ids[i] (HOST, >= 0) is the row's Philox row index: a sampled row draws what row row_ids[i] of a batch begun together draws.  max_new, eos,
 * sampling, processors, constraints and log-probabilities are the running batch's.  After an admission trace_decode_steps' bound is per row: a call is
 * refused only when no row has n steps of its own left; a row past its max_new is stepped on without recording or advancing (it rewrites the last
 * cache row its own slot allows).  The next trace_decode_steps runs the step of the new batch size.  Returns after the stream has run the copies.
 * TRACE_ERR_STATE: no batch running; host-select mode; a shared prefix is live (trace_decode_set_shared_prefix); a slot not prefilled.
 * TRACE_ERR_ARG: B + n above the cap of trace_decode_begin; a slot the batch holds, or twice in the list; prefill + max_new > max_ctx; a head outside
 * 0..2; a negative row index; forced ids while processors or constraints are armed.  After one of these errors, all of them found by the argument
 * and state checks before anything is queued, the batch is as it was.  A copy or launch that fails after them (a HIP error) leaves B and the B
 * running rows' state and the shared counter untouched, but rows [B, B + n) of the per-row arrays and the spare counter pair are already written:
 * harmless for the running rows, not "as it was". */
int trace_decode_admit(trace_ctx* ctx, const int32_t* slots, int n, const int32_t* heads, const int32_t* row_ids, const int32_t* forced, void* stream);
/* Host-driven token selection (do_sample=True in scripts/inference/inference.py:62, stopping criteria): with host
 * mode on (set before trace_decode_begin), begin/steps stop after the masked head logits; the host picks the ids and
 * trace_decode_feed applies them (output record, head switch, next-token embedding).  One eager step at a time. */
int trace_decode_host_mode(trace_ctx* ctx, int on);
int trace_decode_feed(trace_ctx* ctx, const int32_t* tokens, int B, void* stream);

/* Sampling (generate(do_sample=True): HF TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> multinomial, transformers 4.40.1),
 * on the device.  Set before trace_decode_begin; it holds for every later batch until changed.  temperature <= 0 = greedy (the arg-max path,
 * unchanged).  Otherwise every token is drawn from the masked fp32 logits of the row's active head [lo, hi) (the text head includes <sync>):
 *   1. x = logit / temperature (fp32 division);
 *   2. top_k in [1, 1024]: keep x >= the k-th largest x (ties at the threshold kept; k >= the head's width keeps all).  top_k = 0 = off;
 *   3. top_p in (0, 1]: order the kept tokens by (x desc, id asc) and keep a token iff the probability mass ranked strictly above it is < top_p
 *      (the top token always stays);
 *   4. draw u in [0, 1) and walk the kept tokens in that order (top_k = 0: the whole head in id order) accumulating exp(x - max): the first token
 *      whose running sum exceeds u * total (the last kept token if rounding leaves none).
 * RNG contract: u = (x >> 8) * 2^-24 with x = word 0 of Philox4x32-10 under key = seed (64 bits), counter = (step, 0, b, 0), where step is the
 * device step counter (0 = the token of trace_decode_begin) and b the row within the decode batch — the first rocrand() after
 * rocrand_init(seed, b, 4 * step) of rocrand_philox4x32_10.h.  Identical inputs and seed give identical ids, eager or graph-replayed.
 * Domain: top_k in [1, 1024] with any top_p, or top_k = 0 with top_p = 1; anything else (and a NaN / infinite temperature) -> TRACE_ERR_ARG.
 * Forced ids, EOS and the head switch behave as in greedy decoding; host-select mode (trace_decode_host_mode) ignores the setting.
 * The params live in device memory: a captured decode step (use_graph) stays valid when they change between calls. */
int trace_decode_set_sampling(trace_ctx* ctx, float temperature, int top_k, float top_p, uint64_t seed);

/* The same with HF's remaining sampling warpers, applied between step 3 and the draw in HF's order (min_tokens_to_keep = 1 throughout); each sees
 * the distribution renormalised over what the steps before it kept:
 *   3a. min_p in [0, 1] (0 = off): drop p < min_p * p_max;
 *   3b. typical_p in (0, 1] (1 = off): H = -sum p log p; order the tokens by |-log p - H| ascending; last = the number of tokens whose inclusive
 *       cumulative probability in that order is < typical_p (at most the last index); keep every token whose |-log p - H| is <= that of the token
 *       at `last` (equal values stay together).  This can drop the arg-max;
 *   3c. epsilon_cutoff in [0, 1) (0 = off): drop p < epsilon_cutoff; tokens equal to the maximum always stay;
 *   3d. eta_cutoff in [0, 1) (0 = off): eta = min(eta_cutoff, sqrt(eta_cutoff) * exp(-H)), H of the distribution it receives; drop p < eta; tokens
 *       equal to the maximum always stay.
 * The draw then walks what is left in the order of step 4.  size = sizeof(trace_sampling) as the caller compiled it (a smaller one -> TRACE_ERR_ARG).
 * temperature <= 0 = greedy (the other fields are not read).  Domain: that of trace_decode_set_sampling, and top_k in [1, 1024] as soon as one of
 * the four is armed; anything else -> TRACE_ERR_ARG.  With the four off it is trace_decode_set_sampling: the same ids from the same rows.
 * trace_decode_set_sampling itself means "the four off". */
typedef struct trace_sampling {
    int32_t size;
    float temperature;
    int32_t top_k;
    float top_p;
    uint64_t seed;
    float min_p, typical_p, epsilon_cutoff, eta_cutoff;
} trace_sampling;
int trace_decode_set_sampling_ex(trace_ctx* ctx, const trace_sampling* sampling);

/* Per-token log-probabilities, computed on the device inside the decode step.  Set before trace_decode_begin; it holds for every later batch
 * until changed (like trace_decode_set_sampling).  The first call with on != 0 allocates the masked-logits rows and [256][max_new_tokens] floats.
 * For row b at step s, with head = the row's active head at that step, [lo, hi) its id range, and x the RAW masked fp32 logits of that range as
 * the head stage writes them (no temperature, no top-k, no top-p: the model's distribution, not the warped one):
 *     logprob[b][s] = (x[id] - M) - log(S),   M = max x,   S = sum_i exp(x_i - M)
 * id = the token recorded in out_ids[b][s] (under forced ids: the model's own choice — trace_llm_score_append scores the fed ids; an id outside [lo, hi) gives -inf).  S is formed exactly
 * as the sampler forms its sums: weights from the sampler's exp, thread t of 256 sums the id-order run [t C, (t + 1) C), C = ceil((hi - lo) / 256),
 * then a Hillis-Steele scan over the 256 run totals; no FMA contraction anywhere.  log (arguments >= 1: the maximum contributes exp(0)) is
 * the odd atanh series of csrc/sample.h sample_log, every operation rounded on its own.  trace_amd/sampling.py token_logprob_ref restates it
 * in float32 and reproduces the device value bit for bit; greedy or sampled, eager or graph-replayed, the value is the same.
 * Entries past a row's length are 0.0, so a plain sum over a row is the sequence score; the EOS token's entry is included.
 * Host-select mode (trace_decode_host_mode) computes nothing: the host holds the logits and calls trace_op_token_logprob on them.
 * With the setting off a decode batch issues the launches and replays the graphs it did before (steps with the extra launch are cached apart).
 * trace_decode_read_logprobs: synchronises and copies [B, max_new] floats to a HOST buffer; TRACE_ERR_STATE if the current batch was begun
 * without log-probabilities. */
int trace_decode_set_logprobs(trace_ctx* ctx, int on);
/* Shared prompt prefix of a decode batch: every slot the NEXT trace_decode_begin is given holds the same K / V rows at positions [0, rows) (a batch
 * prefilled through trace_llm_prefill_shared, or copies made by trace_kv_copy), and `slot` is one that holds them.  The decode attention then reads
 * those positions of every sequence from that one slot — one copy that stays in cache instead of B from memory; ids, heads and log-probabilities are
 * bit-identical to the unshared batch.  Whole 32-position blocks only: rows is floored to a multiple of 32; rows < 32 or slot < 0 = off.  The
 * request is consumed by the next trace_decode_begin (which answers TRACE_ERR_ARG if a sequence is shorter than the shared rows, TRACE_ERR_STATE if
 * the slot is); a begin with no request before it decodes unshared.  A batch of one never shares.  Steps captured for another (slot, rows) pair are
 * cached apart (two pairs per batch size).  TRACE_ERR_ARG: slot / rows out of range; TRACE_ERR_STATE: an e4m3 KV cache. */
int trace_decode_set_shared_prefix(trace_ctx* ctx, int slot, int rows);
int trace_decode_read_logprobs(trace_ctx* ctx, float* out, void* stream);

/* Logits processors (generate(repetition_penalty=, no_repeat_ngram_size=, min_new_tokens=): HF RepetitionPenaltyLogitsProcessor ->
 * NoRepeatNGramLogitsProcessor -> MinNewTokensLengthLogitsProcessor, transformers 4.40.1), on the device inside the decode step.  Set before
 * trace_decode_begin; it holds for every later batch until changed (like trace_decode_set_sampling); (1.0, 0, 0) disarms it.  The first arming call
 * allocates the processed-logits rows, and the masked-logits rows if nothing has allocated them yet.  For row b at device step s (0 = the token of
 * trace_decode_begin), with [lo, hi) the id range of the row's active head and x its masked fp32 logits as the head stage writes them:
 *   history h = the ids the row has recorded so far, out_ids[b][0 .. out_len[b]).  The prompt is NOT part of it (the reference hands HF
 *     inputs_embeds, so HF's processors see the generated ids only).  Ids are global vocabulary ids [text | <sync> | time | score]: a time digit
 *     emitted in one time span is penalised / banned in a later one as well, as HF does on the reference.  Ids of h outside [lo, hi) touch nothing.
 *   1. repetition_penalty p (> 0, finite; 1.0 = off; p < 1 rewards): for every DISTINCT id t of h: x[t] = x[t] < 0 ? x[t] * p : x[t] / p — one fp32
 *      multiply or one true fp32 division of the raw value, once per id however often it occurs; -inf stays -inf, 0 stays 0;
 *   2. no_repeat_ngram_size n (0 = off, 1..64): if len(h) + 1 >= n, for every i in [0, len(h) - n] with h[i .. i+n-2] == h[len(h)-n+1 .. len(h)-1]:
 *      x[h[i+n-1]] = -inf (n = 1 bans every id of h);
 *   3. min_new_tokens m (0 = off): while s < m and eos >= 0: x[eos] = -inf, eos the one given to trace_decode_begin.
 * The three rules are independent and commute.  The token is then selected from the processed row: the arg-max with the lowest id among equal
 * maxima, or the sampler above.  If every id of the head ends up banned, greedy emits the head's lowest id; under sampling that case is unspecified.
 * Log-probabilities (trace_decode_set_logprobs) stay what they were: they describe the RAW row, the model's own distribution — the processed row
 * lives in a buffer of its own.  Rows that are done keep stepping; nothing is recorded for them.  With the setting off a decode batch issues the
 * launches and replays the graphs it did before (steps with the extra launch are cached apart); the params live in device memory, so a captured
 * step stays valid when they change between batches.  Host-select mode (trace_decode_host_mode) ignores the setting: the host holds the logits and
 * calls trace_op_logits_process on them.  TRACE_ERR_ARG: p <= 0 or not finite, n outside 0..64, m < 0; and, at trace_decode_begin, an armed
 * setting together with forced != NULL (the history is the recorded ids, which under forced ids are not the fed ones). */
int trace_decode_set_logits_params(trace_ctx* ctx, float repetition_penalty, int no_repeat_ngram_size, int min_new_tokens);

/* Per-row generation parameters.  One trace_row_params per row of a decode batch: the row's own sampling (its own seed included), its own logits
 * processors and its own max_new, so that a greedy request, a sampled one and a 16-token one next to a 512-token one share one running batch.
 * trace_decode_set_row_params hands rows [n] (HOST) to the NEXT trace_decode_begin, whose B must equal n (else TRACE_ERR_ARG from that begin); that
 * begin consumes the request whatever it answers.  NULL or n == 0 = off: a batch begun without a request is what it has always been, launch for launch.
 * size = sizeof the struct as the caller compiled it, the same in every entry and the stride of the array; smaller than this library's -> TRACE_ERR_ARG.
 * Domain per row: `sampling` as trace_decode_set_sampling_ex takes it (temperature <= 0: this row is greedy and the rest of `sampling` is not read;
 * the nested size field is read for a sampled row), the three processors as trace_decode_set_logits_params takes them, max_new in 1 .. the max_new
 * given to trace_decode_begin.  Everything else -> TRACE_ERR_ARG: domain errors from trace_decode_set_row_params itself (max_new there against the
 * context's max_new_tokens), a max_new above the batch's from the begin.
 * What a per-row batch does: the selection reads row b's params — a sampled row draws as under trace_decode_set_sampling_ex with ITS seed at
 * counter (the row's own step, 0, its Philox row index, 0); a greedy row takes the arg-max over its head range, the lowest id among equal maxima —
 * and the row's own max_new bounds what it records, feeds from `forced`, advances and log-scores; the max_new of the begin stays the stride of the
 * ids / forced / log-probability rows and of trace_decode_read.  A row that has recorded its own max_new ids is stepped on without recording or
 * advancing, as a row past max_new is after an admission.  trace_decode_steps is refused only when no row has n steps of its own left, and
 * prefill + the row's own max_new must fit max_ctx.  The logits processors' launch runs when any row's processors or a ban rule of the constraints is
 * armed (decided at begin and at every admission).  Such a batch captures its steps into graph places of its own.
 * Everything else stays batch-wide: a per-row batch ignores trace_decode_set_sampling / _ex and trace_decode_set_logits_params; eos, the constraints,
 * the log-probabilities switch and the shared prefix are the batch's.  Forced ids are refused (TRACE_ERR_ARG) only for a row whose processors are
 * armed and that is fed an id within its own max_new, or for any row when constraints are armed.  Host-select mode: TRACE_ERR_STATE (from the
 * setter, and from a begin that finds a request).  trace_decode_retire moves a row's params with the row.
 * trace_decode_admit_ex is trace_decode_admit with rows [n] (HOST) for the admitted rows, written before their token 0 is selected.  Rows go into a
 * batch begun with row params only through it with rows != NULL (trace_decode_admit, which is _ex with rows == NULL, answers TRACE_ERR_STATE there);
 * rows != NULL into a batch begun without them is TRACE_ERR_STATE.  Its other errors are trace_decode_admit's, with the row's own max_new in the
 * max_ctx check.  After an error the batch is as it was: all argument and state checks come before anything is queued, as in trace_decode_admit. */
typedef struct trace_row_params {
    int32_t size;
    trace_sampling sampling;
    float repetition_penalty;
    int32_t no_repeat_ngram_size, min_new_tokens;
    int32_t max_new;
} trace_row_params;
int trace_decode_set_row_params(trace_ctx* ctx, const trace_row_params* rows, int n);
int trace_decode_admit_ex(trace_ctx* ctx, const int32_t* slots, int n, const int32_t* heads, const int32_t* row_ids, const int32_t* forced,
                          const trace_row_params* rows, void* stream);

/* Constraints (generate(bad_words_ids=, suppress_tokens=, begin_suppress_tokens=, stop_sequences=, eos_token_id=[a, b, ...])): HF
 * NoBadWordsLogitsProcessor, SuppressTokensLogitsProcessor, SuppressTokensAtBeginLogitsProcessor and id-level stop sequences, on the device inside
 * the decode step.  Notation as above: row b, device step s, head range [lo, hi), history h = out_ids[b][0 .. out_len[b]): generated ids only, as
 * global vocabulary ids; it never holds the prompt.  The ban rules write -inf into the processed row, after rule 2 above, so a ban overwrites a
 * penalised value:
 *   4. bad_words: for every sequence w of k ids: k == 1: x[w[0]] = -inf; k > 1: if len(h) >= k - 1 and the last k - 1 ids of h equal
 *      w[0 .. k-1): x[w[k-1]] = -inf.  The prefix comparison is over global ids whatever head emitted them: a bad word may cross heads (text id,
 *      <sync>, time digit).
 *   5. suppress: x[t] = -inf for every listed t, at every step.
 *   6. begin_suppress: the same at s == 0 only (HF's begin_index is 0 when generate() is handed inputs_embeds, as the reference does).
 *   3. (widened) while s < min_new_tokens: eos and the id of every stop sequence of length 1 are banned: HF bans every id of its EOS list.
 * An id to ban outside [lo, hi) touches nothing.
 * Stop rule, in the selection, after the step's token is recorded for a row that was not done: a stop sequence w of k ids fires iff
 * out_len[b] >= k and the last k recorded ids equal w; the row is then done exactly as an EOS row is.  The stop ids stay in the row's output and
 * out_len counts them, as with EOS.  Matching is over global ids and never reaches into the prompt or another row's history.  A done row keeps
 * stepping and records nothing.  Several EOS ids are stop sequences of length 1.
 * Bounds: at most 64 stop sequences and 64 bad-word sequences of 1..32 ids each, at most 1024 ids in each suppress list; every id inside
 * [0, V+1+Tv+Sv).  Anything else is TRACE_ERR_ARG, before any launch; nothing is truncated.
 * trace_constraints: size = sizeof(trace_constraints) of the caller; the two sequence lists in CSR form (offsets of n + 1 entries, offsets[0] = 0,
 * sequence i = ids[offsets[i] .. offsets[i+1])); all pointers are host pointers, read during the call only.
 * trace_decode_set_constraints: NULL or all counts zero disarms.  Set before trace_decode_begin; it holds for every later batch until changed.  The
 * first arming call allocates the device table, and the masked / processed logits rows if nothing has allocated them yet.  The table is copied to
 * device memory at trace_decode_begin and read from there, so a captured step stays valid when it changes between batches; steps with the stop
 * match are cached apart, and with nothing armed a batch issues the launches and replays the graphs it did before.  Log-probabilities keep
 * describing the RAW row.  Host-select mode ignores the setting (the host calls trace_op_logits_process_ex / trace_op_stop_match).  An armed
 * setting together with forced != NULL is TRACE_ERR_ARG at trace_decode_begin, as for the logits params. */
typedef struct trace_constraints {
    int32_t size;
    int32_t n_stop, n_bad_words, n_suppress, n_begin_suppress;
    const int32_t* stop_offsets;        /* n_stop + 1 */
    const int32_t* stop_ids;
    const int32_t* bad_word_offsets;    /* n_bad_words + 1 */
    const int32_t* bad_word_ids;
    const int32_t* suppress_ids;
    const int32_t* begin_suppress_ids;
} trace_constraints;
int trace_decode_set_constraints(trace_ctx* ctx, const trace_constraints* constraints);

/* Two-stage pipeline support (trace/eval/evaluate.py:298-417 loops over independent videos: while one batch decodes — HBM-bound —
 * the next batch's ViT + prefill — MFMA-bound — can run on another stream into other KV slots; the stages share no buffers).
 * trace_stream_create: a HIP stream confined to cu_count CUs starting at logical CU cu_first (hipExtStreamCreateWithCUMask; mask bit i
 * is CU i / 8 of XCD i % 8, so a run of bits is spread evenly over the XCDs; cu_first and cu_count multiples of 8); cu_count == 0: an
 * ordinary non-blocking stream.  A CU-masked stream's persistent GEMMs launch at most cu_count workgroups (one per CU the stream can use);
 * trace_set_gemm_cus overrides that number for the streams this context has created (n workgroups; 0 = the device's CU count) — it is a
 * property of those streams and goes away with them.  Streams are destroyed with trace_stream_destroy (idle). */
int trace_stream_create(trace_ctx* ctx, int cu_first, int cu_count, void** stream_out);
int trace_stream_destroy(trace_ctx* ctx, void* stream);
int trace_set_gemm_cus(trace_ctx* ctx, int n);

/* Timing hook for bench.py: average device time (ms, hipEvents on `stream`) of the last trace_decode_steps call
 * per step, and of its skinny-GEMM launches if profiling was enabled with trace_set_profile(ctx, 1). */
int trace_set_profile(trace_ctx* ctx, int on);
/* Debugging aid: device addresses of the K cache, the V^T cache and the prefill's last-position hidden rows, with strides[8] = layer, slot, kv-head
 * strides (elements), ctx_pad, layers, kv heads, head_dim, hidden (tools/pipeline_stress.py checksums them between the pipeline's stages). */
int trace_debug_buffers(trace_ctx* ctx, void** kcache, void** vcache, void** xlast, int64_t* strides);
/* The batch sizes a captured decode step exists for (any tail mode), ascending, into sizes[0 .. cap) (HOST, may be NULL); returns their number. */
int trace_debug_step_graphs(trace_ctx* ctx, int32_t* sizes, int cap);
/* One per-row column of the running decode batch, rows [0, B), as 32-bit words into out[0 .. cap) (HOST); synchronous.  Returns the column's words per
 * row, or 0 with nothing written where the armed mode has no such column (logprobs; the per-row params).  trace_debug_decode_column(ctx, i) names
 * column i (slots, pos, heads, done, out_len, row_id, step0, out_ids, forced, logprobs, row_sp, row_lp, row_max, x), NULL past the end. */
int trace_debug_decode_rows(trace_ctx* ctx, int column, int32_t* out, int cap);
const char* trace_debug_decode_column(trace_ctx* ctx, int i);
/* The same for a kv_cache_fp8 context: device addresses of K8, V8 (bytes), ks, vs (fp32), strides[8] = layer, slot, kv-head strides of the payload in
 * BYTES (those of the scales are these / 128), ctx_pad, layers, kv heads, head_dim, hidden.  TRACE_ERR_STATE on a 16-bit-cache context. */
int trace_debug_kv8_buffers(trace_ctx* ctx, void** k8, void** v8, void** ks, void** vs, int64_t* strides);
/* out[0..n) (n <= 20): [0] ms per decode step of the last trace_decode_steps call, [1] its steps, [2] average ms of the bracketed decode launch,
 * [3] its samples, [4] its algorithmic bytes, [5] average ms of the bracketed ViT fc1 GEMM launch, [6] its samples, [7] its GFLOP,
 * [8] which decode launch took the bracket: 1 = gate|up GEMV, 2 = batch-1 fused-norm gate|up GEMV, 3 = the layer-0 decode attention (the wide step's
 * own choice, or bracket bit 2), 4 = the layer-0 append launch (bracket bit 3),
 * [9] always 0 (rounds 3-4: whether the bracketed ViT GEMMs ran with the LayerNorm fold; the fold left the product in round 5),
 * [12..14] average ms of the bracketed ViT qkv / out-proj / fc2 GEMM launches (layer 0, the same calls as [5]), [15..17] their GFLOP. */
int trace_get_profile(trace_ctx* ctx, float* out, int n);
/* Which per-launch brackets profiling mode 2 takes: bit 0 = the ViT fc1 GEMM, bit 1 = the decode step's dominant kernel; instead of bit 1 (set one
 * of the three), bit 2 = the layer-0 decode attention in whichever step body runs (with its fused append where it has one; [4] = the K + V bytes it streams),
 * bit 3 = the layer-0 append launch (qkv_finish / qkv_finish_kv8; none is taken where the step fuses the append into the attention).  A pipelined caller
 * (two stages on two streams) leaves a stage's bracket on only while that stage has the GPU to itself (pipeline fill / drain). */
int trace_set_profile_brackets(trace_ctx* ctx, int mask);

/* ---- kernel-level entry points (unit tests / microbenchmarks; raw device pointers) ---- */
int trace_op_gemm(const void* A, int lda, const void* W, int ldw, void* C, int ldc, const void* bias, const void* R,
                  int ldr, int M, int N, int K, int epilogue, void* stream);
/* The process-wide A/B switches of the kernel launchers, by name ("gemm.kernel", "decode.wide_min_rows", "attn.vit.big", ...: engine.hip TUNE_ROWS holds
 * every name with its range, default and meaning; trace_op_tuning_name(i) enumerates them, NULL past the end).  set: TRACE_ERR_ARG for an unknown name or a
 * value outside the field's range; reset: every field back to its default.  For tests and tools: not while launches are in flight. */
int trace_op_tuning_set(const char* name, int value);
int trace_op_tuning_get(const char* name, int* value);
int trace_op_tuning_reset(void);
const char* trace_op_tuning_name(int i);
/* The same switches by their older numeric codes: 0-8 = gemm.kernel (0 auto, 2 = 128^2 tiles, 3 = 256^2 tiles (gemm.hip), 4 = gemm_ldr.hip, 5-7 = gemm_pers.hip
 * ticketed / static deal / one tile per workgroup, 8 = gemm_w4.hip); every other range is a row of engine.hip LEGACY_CODES. */
int trace_op_set_gemm_variant(int variant);
/* Which kernel trace_op_gemm runs this shape on under the current tuning values, without launching (no GPU needed): 0 = 128^2 tiles, 1 = 256^2 tiles (gemm.hip),
 * 2 = gemm_ldr.hip, 3 = gemm_pers.hip, 4 = gemm_w4.hip, | the persistent kernels' tile walk << 8 (0 ticketed, 1 static deal, 2 one workgroup per tile);
 * TRACE_ERR_ARG for a shape trace_op_gemm rejects. */
int trace_op_gemm_route(int M, int N, int K, int lda, int ldw, int ldc, int ldr, int epilogue, int fp8);
/* profiling: device buffer of 8 x uint64 per workgroup receiving phase time stamps of every later GEMM launch (NULL = off) */
int trace_op_set_gemm_trace(void* buf);
int trace_op_layernorm(const void* x, void* y, const void* w, const void* b, int rows, int D, float eps, void* stream);
int trace_op_rmsnorm(const void* x, void* y, const void* w, int rows, int D, float eps, void* stream);
/* The same two with what the engine's call sites use: row strides ldx / ldy (elements, multiples of 8; y may be x), and for the LayerNorm silu = 1
 * (y = SiLU(el(LN(x)))) and res / ldres (y = act(el(LN(x)) + res), y may be res; NULL = none) — el() rounds to the 16-bit element type first. */
int trace_op_layernorm_ex(const void* x, int ldx, void* y, int ldy, const void* w, const void* b, int rows, int D, float eps, int silu,
                          const void* res, int ldres, void* stream);
int trace_op_rmsnorm_ex(const void* x, int ldx, void* y, int ldy, const void* w, int rows, int D, float eps, void* stream);
/* The STC connector's row kernels, each alone, as trace_stc_connector calls them.  Channels-last rows of the 16-bit element type, contiguous;
 * fp32 arithmetic, one rounding at the store.  TRACE_ERR_ARG, before any launch, for a null tensor, a non-positive extent, a C that is not a
 * positive multiple of 8 (64 for the pool) or an act outside 0..3.
 *   dwconv3x3          y [N, H, W, C] = depthwise 3 x 3, pad 1, stride 1 of x [N, H, W, C]; w [C, 9] (Conv2d weight [C, 1, 3, 3])
 *   avgpool            y [N, C] = mean over the HW pixels of x [N, HW, C] (N <= 65535)
 *   bias_act           x [rows, C] = act(x + bias) in place; bias [C] or NULL; act 0 none, 1 SiLU, 2 sigmoid, 3 GELU (exact erf form)
 *   scale_rows         x [N, HW, C] *= gate [N, C] in place
 *   im2col3d           A [To Ho Wo, 8 C] = the 2 x 2 x 2 patches of x [T, H, W, C] for Conv3d(kernel 2, stride 2, padding 1): To = T / 2 + 1 (Ho, Wo
 *                      alike), column ((kt 2 + kh) 2 + kw) C + c = x[2 to - 1 + kt][2 yo - 1 + kh][2 xo - 1 + kw][c], zero outside x (zeros are written)
 *   permute_conv3d_w   out [Co, 8, Ci] = Conv3d weight w [Co, Ci, 2, 2, 2] in im2col3d's column order (tap = (kt 2 + kh) 2 + kw) */
int trace_op_dwconv3x3(const void* x, const void* w, void* y, int N, int H, int W, int C, void* stream);
int trace_op_avgpool(const void* x, void* y, int N, int HW, int C, void* stream);
int trace_op_bias_act(void* x, const void* bias, int64_t rows, int C, int act, void* stream);
int trace_op_scale_rows(void* x, const void* gate, int N, int HW, int C, void* stream);
int trace_op_im2col3d(const void* x, void* A, int T, int H, int W, int C, void* stream);
int trace_op_permute_conv3d_w(const void* w, void* out, int Co, int Ci, void* stream);
/* SpatialSlotPool before `readout` (trace_slot_pool without its GEMM): feats + t * frame_stride + p * row_stride is patch p of frame t (elements;
 * frame_stride a multiple of 8, row_stride a multiple of 8 and >= D), ln_w / ln_b [D], slots [D, 8], cos_t / sin_t fp32 [n, D / 2] (the caller's
 * tables), res_out [T, 8, D], D a multiple of 16 up to 1024.  ws: trace_op_slot_pool_ws_floats(T, D) floats of device scratch. */
int64_t trace_op_slot_pool_ws_floats(int T, int D);
int trace_op_slot_pool(const void* feats, int64_t frame_stride, int row_stride, const void* ln_w, const void* ln_b, const void* slots,
                       const float* cos_t, const float* sin_t, void* res_out, int T, int n, int D, float eps, float* ws, int64_t ws_floats,
                       void* stream);
/* The fused ViT front end from checkpoint-layout tensors, run as the load and forward paths run it (weight repack, CLS row, patch-embed kernel):
 * frames [T, 3, S, S] (frames_dtype as in trace_vit_forward), conv_w [D, 3 P P], cls [D], pos [G G + 1, D] (G = S / P), pre_layrnorm weight / bias
 * [D] -> X_out [T, G G + 1, D].  ws: trace_op_patch_embed_ws_elems(P, D) 16-bit elements of device scratch.  TRACE_ERR_ARG for a geometry the
 * fused kernel does not take (P outside {14, 16}, S % P != 0, D outside {128, 256, 512, 1024}) — there the engine runs im2col + GEMM + assemble. */
int64_t trace_op_patch_embed_ws_elems(int P, int D);
int trace_op_patch_embed(const void* frames, int frames_dtype, const void* conv_w, const void* cls, const void* pos, const void* pre_w,
                         const void* pre_b, void* X_out, int T, int S, int P, int D, float eps, void* ws, int64_t ws_elems, void* stream);
int trace_op_attention(const void* Q, const void* K, const void* V, void* O, void* vt_scratch, int batch, int heads,
                       int kv_heads, int nq, int nkv, int head_dim, int causal, float scale, void* stream);
/* Decode GEMV out[b,n] = sum_k X[b,k] W[n,k], B <= 64.  w_tiled: W in the decode tile layout written by
   trace_op_tile_pack ([N/16][K/64][64][16]) instead of row-major.  epilogue 0 none, 1 +R, 3 SwiGLU (16-row interleaved
   gate|up), 4 partial: `out` = fp32 k-chunk partial rows [trace_op_skinny_ks()][trace_op_sk_rows()][N] for trace_op_add_rmsnorm. */
int trace_op_skinny_gemm(const void* X, const void* W, void* out, const void* R, int B, int N, int K, int epilogue,
                         int w_tiled, void* stream);
int trace_op_skinny_ks(int N, int K, int epilogue, int B);
/* How the decode GEMV of one kind (0 = bf16 weights: trace_op_skinny_gemm, 1 = e4m3 weights and activations: trace_op_skinny_fp8, 2 = e4m3 weights, bf16
   activations: trace_op_skinny_w8; these two take epilogue 4 only) is cut into workgroups, without launching (no GPU needed; without one the plan is the
   256-CU MI355X's): out[0..11) = k-chunks KS (= trace_op_skinny_ks for kind 0), k-units per chunk (64 k of bf16, 128 k of e4m3), tiles per workgroup T,
   waves per tile, tiles, grid, threads, 16-row output tiles per task NT, 16-row activation groups NB, dynamic LDS bytes, and the floats of partial rows
   that hold epilogue 4's product of this N, K at any B (KS * trace_op_sk_rows() * N at its largest).  TRACE_ERR_ARG for a shape the kind's GEMV rejects. */
int trace_op_skinny_plan(int kind, int N, int K, int epilogue, int B, int64_t* out);
/* What one decode step of B sequences does on a decoder of this geometry (fp8_scheme: trace_config.llm_weights_fp8) under the current tuning values,
   without launching: out[0..8) = the step body (1 GEMV step, 2 fused-norm GEMV step, 3 wide GEMM step: trace_get_profile's [8]), the GEMV kind as above,
   1 if RoPE + cache append run as a launch of their own, the k-chunks of the qkv / o / gate|up / down partial rows (gate|up: 0 on the wide step), the
   attention's context splits.  TRACE_ERR_ARG for B outside 1..trace_op_sk_rows() and for an fp8 scheme with B > 64. */
int trace_op_decode_route(int B, int fp8_scheme, int H, int I, int QKV, int32_t* out);
/* Decode GEMV of 1..4 rows with the preceding "sum the partial rows + residual -> new residual, RMSNorm" folded in: part_in [ks_in][sk_rows][K] fp32
   (ks_in may be 0) + R [B,K] -> xout [B,K]; out = fp32 partial rows [trace_op_skinny_ks(N,K,4,B)][sk_rows][N] of RMSNorm(xout; w, eps) . W^T */
int trace_op_skinny_fused_norm(const float* part_in, int ks_in, const void* R, void* xout, const void* w, float eps, const void* W, float* out,
                               int B, int N, int K, void* stream);
/* trace_op_skinny_plan / trace_op_decode_route for w4 weights (kind 3: e2m1 codes + block exponents, bf16 activations; units of 256 k; epilogue 4
   only), without launching: the same out[0..11) / out[0..8).  The GEMV takes K % 256 == 0, N % 16 == 0, B <= 64; the route H % 256 == 0, I % 256 == 0. */
int trace_op_skinny_w4_plan(int N, int K, int B, int64_t* out);
int trace_op_decode_route_w4(int B, int H, int I, int QKV, int32_t* out);
int trace_op_sk_rows(void);                 /* row stride of every fp32 partial-row buffer = the largest decode batch (256) */
/* Decode batches above 64 rows: out = X[M <= 128, K] . W[N, K]^T (row-major W) as fp32 k-chunk partial rows
   [trace_op_gemm_partial_ks(N, K)][trace_op_sk_rows()][N] for trace_op_add_rmsnorm (split-K MFMA GEMM, 128x128 tiles) */
int trace_op_gemm_partial_ks(int N, int K);
int trace_op_gemm_partial(const void* A, const void* W, float* part, int M, int N, int K, int w_tiled, void* stream);
/* w_tiled: W is the trace_op_tile_pack copy (1; 5 = with the 4-stage K-tile ring the engine uses).  The gate|up product of such a step: tiled 16-row interleaved
   gate|up matrix, SwiGLU epilogue, out [M, N/2] bf16 */
int trace_op_gemm_swiglu_tiled(const void* X, const void* Wt, void* out, int M, int N, int K, int ring, void* stream);
int trace_op_tile_pack(const void* W, void* Wt, int N, int K, void* stream);
/* fp8 path pieces: row quantiser (X bf16 [rows,K] -> e4m3 bytes + scale[row] = amax/448), the W8A8 GEMM
   C = (A8 . W8^T) * sa[m] * sw[n] (+ residual / SwiGLU epilogue as trace_op_gemm), and the decode GEMV (fp32 out [B,N]) */
int trace_op_quant_rows_fp8(const void* X, void* X8, float* sx, int rows, int K, void* stream);
int trace_op_gemm_fp8(const void* A8, const float* sa, const void* W8, const float* sw, void* C, const void* R, int M, int N, int K,
                      int epilogue, void* stream);
int trace_op_skinny_fp8(const void* X8, const float* sx, const void* W8, const float* sw, float* out, int B, int N, int K, void* stream);
/* the weight-only decode GEMV: X bf16 [B,K] . (e4m3 W8 [N,K] widened to bf16)^T * sw[n] -> fp32 out [B,N] */
int trace_op_skinny_w8(const void* X, const void* W8, const float* sw, float* out, int B, int N, int K, void* stream);
/* out[b][j] = bf16(silu(sum_ks gate) * sum_ks up) from partial rows [KS][trace_op_sk_rows()][N2] of the 16-row interleaved gate|up GEMV */
int trace_op_swiglu_combine(const float* part, int KS, int N2, void* out, int B, void* stream);
/* x = bf16(sum_ks part[ks][b][:]) + R[b][:] -> xout;  y = RMSNorm(x) * w   (decode residual add + norm, N <= 4096) */
int trace_op_add_rmsnorm(const float* part, int KS, const void* R, void* xout, const void* w, void* y, int B, int N,
                         float eps, void* stream);
/* The same kernel as the decode step calls it: row strides ldr / ldx / ldy (elements, multiples of 4), xout may be R (in place, the engine's form),
   KS chunks read of part [>= KS][trace_op_sk_rows()][N], and y8 [B][N] e4m3 bytes + sy [B] fp32 = the rule of trace_op_quant_rows_fp8 applied to
   y (both NULL: not written; one NULL: TRACE_ERR_ARG).  TRACE_ERR_ARG before any launch: N % 4, N > 4096, B outside 1..trace_op_sk_rows(), KS < 1,
   a stride that is no multiple of 4 or below N, and y8 / sy in the fp16 library (it has no fp8 weight path). */
int trace_op_add_rmsnorm_ex(const float* part, int KS, const void* R, int ldr, void* xout, int ldx, const void* w, void* y, int ldy, void* y8,
                            float* sy, int B, int N, float eps, void* stream);
/* The down GEMV of 1..4 rows with SwiGLU folded in: part_gu [ks_gu][sk_rows][2 K] fp32 (partial rows of the 16-row interleaved gate|up GEMV) ->
   out = fp32 partial rows [trace_op_skinny_ks(N,K,4,B)][sk_rows][N] of el(silu(sum gate) * sum up) . W^T (W row-major [N][K]; packed internally).
   TRACE_ERR_ARG: B outside 1..4, K % 64, N % 16, N < 16, ks_gu < 1, a null argument. */
int trace_op_skinny_fused_swiglu(const float* part_gu, int ks_gu, const void* W, float* out, int B, int N, int K, void* stream);
/* kcache [B, nkv, max_ctx, 128] row-major; vtcache [B, nkv, 128, max_ctx] = V transposed (the engine's cache layout,
   max_ctx % 32 == 0); pos[b] = newest position, already in both caches; q [B, nq*128] rotated; ws B*nq*nsplit*130 floats.
   The kernel fetches whole 32-position blocks: positions pos[b] + 1 .. the next multiple of 32 are READ (their scores are masked
   and their weights are exactly 0, so what they hold never counts) — both caches must hold finite values there (the engine's
   caches are zero-filled at creation and only ever hold finite values). */
/* The same sampler over loose rows (tests; the host-driven decode loop): logits [B][ld] fp32 device (ld >= V+1+Tv+Sv, masked or not — only the
 * head's range is read), heads / steps int32 [B] device (active head, Philox step), out_ids int32 [B] device = global vocabulary ids.
 * T > 0 and the domain above; row b uses counter (steps[b], 0, b, 0). */
int trace_op_sample(const float* logits, int ld, int B, const int32_t* heads, int V, int Tv, int Sv, float T, int top_k, float top_p,
                    uint64_t seed, const int32_t* steps, int32_t* out_ids, void* stream);
/* trace_op_sample with the four warpers of trace_decode_set_sampling_ex (temperature > 0); trace_op_sample means "the four off". */
int trace_op_sample_ex(const float* logits, int ld, int B, const int32_t* heads, int V, int Tv, int Sv, const trace_sampling* sampling,
                       const int32_t* steps, int32_t* out_ids, void* stream);
/* The log-probability above over loose rows, the same device code: logits [B][ld] fp32 device (only the head's range is read), heads / ids
 * int32 [B] device (active head, global vocabulary id), out fp32 [B] device; an id outside the head's range gives -inf. */
int trace_op_token_logprob(const float* logits, int ld, int B, const int32_t* heads, int V, int Tv, int Sv, const int32_t* ids, float* out,
                           void* stream);
/* The logits processors above over loose rows, the same device code (tests; the host-driven decode loop): logits [B][ld] fp32 device (ld >= V+1+Tv+Sv;
 * only the head's range is read), heads / hist_len / steps int32 [B] device (active head, history length, device step), hist int32 [B][ld_hist]
 * device (row b's history = hist[b][0 .. hist_len[b]), lengths clamped to [0, ld_hist]), eos as trace_decode_begin takes it.  out fp32 [B][ld]
 * device, may not alias logits: the processed values on the head's range, -inf everywhere else of [0, V+1+Tv+Sv).  trace_amd/sampling.py
 * process_row_ref restates a row in float32 bit for bit. */
int trace_op_logits_process(const float* logits, int ld, int B, const int32_t* heads, int V, int Tv, int Sv, const int32_t* hist, int ld_hist,
                            const int32_t* hist_len, const int32_t* steps, int eos, float repetition_penalty, int no_repeat_ngram_size,
                            int min_new_tokens, float* out, void* stream);
/* trace_op_logits_process with the ban rules of a constraint table behind the three processors (rules 4 - 6 and the widened rule 3 of
 * trace_decode_set_constraints; `constraints` NULL = none): the device code the decode step runs.  The stop sequences of the table take part only
 * through rule 3.  The call returns after the stream has run it (the table is staged per call). */
int trace_op_logits_process_ex(const float* logits, int ld, int B, const int32_t* heads, int V, int Tv, int Sv, const int32_t* hist, int ld_hist,
                               const int32_t* hist_len, const int32_t* steps, int eos, float repetition_penalty, int no_repeat_ngram_size,
                               int min_new_tokens, const trace_constraints* constraints, float* out, void* stream);
/* The stop rule over loose histories, the same device code: hist int32 [B][ld_hist] / hist_len int32 [B] device as above; fired_out int32 [B] device:
 * 1 where some stop sequence of `constraints` equals the last ids of hist[b][0 .. hist_len[b]), else 0.  Returns after the stream has run it. */
int trace_op_stop_match(const int32_t* hist, int ld_hist, const int32_t* hist_len, int B, const trace_constraints* constraints, int32_t* fired_out,
                        void* stream);
/* Single-query decode attention over loose caches (head_dim 128, nq == 4 nkv, nkv <= 64, max_ctx % 32 == 0): kcache [B][nkv][max_ctx][128],
 * vtcache [B][nkv][128][max_ctx] (V transposed), row b in slot b; pos[b] (device) = index of the newest token, already in the caches (ctx = pos + 1);
 * q [B][nq * 128] ready (rotated) -> O [B][nq * 128]; ws: B * nq * nsplit * 130 floats.  Cache positions past pos[b] inside a 32-position block are
 * read and must not count: any finite contents are allowed there.  TRACE_ERR_ARG before any launch: B above trace_op_sk_rows(), a shape outside the
 * above. */
int trace_op_attn_decode(const void* q, const void* kcache, const void* vtcache, const int32_t* pos, void* O, float* ws,
                         int B, int nq, int nkv, int max_ctx, int nsplit, float scale, void* stream);
/* The same over caches of num_slots >= B slots (row b in slot b), with positions [0, shared_rows) of EVERY row read from slot shared_slot instead
 * of the row's own (trace_decode_set_shared_prefix; shared_rows floored to a multiple of 32, 0 = trace_op_attn_decode).  TRACE_ERR_ARG before any
 * launch, beyond the above: shared_slot outside [0, num_slots), a position outside [0, max_ctx) or below shared_rows. */
int trace_op_attn_decode_shared(const void* q, const void* kcache, const void* vtcache, const int32_t* pos, void* O, float* ws, int B, int nq,
                                int nkv, int num_slots, int max_ctx, int nsplit, float scale, int shared_slot, int shared_rows, void* stream);
/* The decode step's qkv epilogue as a kernel of its own (the wide step's form): part = the qkv GEMV's fp32 k-chunk partial rows
 * [ks][trace_op_sk_rows()][(nq + 2 nkv) * 128] (q heads | k heads | v heads), summed in chunk order and rounded to the element type; rotate-half RoPE of
 * q and the new k from the caller's tables cos_t / sin_t [max_ctx][64] fp32 at row pos[b]; q_out [B][(nq + 2 nkv) * 128] receives the roped q heads in
 * its first nq * 128 columns (the rest is not written); the K row and the V^T column are stored at position pos[b] of slot slots[b] of
 * kcache [num_slots][nkv][max_ctx][128] / vtcache [num_slots][nkv][128][max_ctx] — nothing else of the caches is written.  slots / pos: int32 [B] device.
 * TRACE_ERR_ARG before any launch: B above trace_op_sk_rows(), a slot outside [0, num_slots) or given twice, a position outside [0, max_ctx). */
int trace_op_qkv_finish(const float* part, int ks, void* q_out, void* kcache, void* vtcache, const int32_t* slots, const int32_t* pos,
                        const float* cos_t, const float* sin_t, int B, int nq, int nkv, int num_slots, int max_ctx, void* stream);
/* The same inputs straight into the decode attention's fused prologue (the narrow step's form): sums, RoPE and the cache append as above, then the
 * attention over positions 0 .. pos[b] of slot slots[b], the new row included -> O [B][nq * 128].  Same sums and roundings as trace_op_qkv_finish
 * followed by trace_op_attn_decode.  ws and the errors as above. */
int trace_op_attn_decode_fused(const float* part, int ks, void* kcache, void* vtcache, const int32_t* slots, const int32_t* pos, const float* cos_t,
                               const float* sin_t, void* O, float* ws, int B, int nq, int nkv, int num_slots, int max_ctx, int nsplit, float scale,
                               void* stream);

/* ---- The e4m3 KV cache format ("kv8"), and its kernels over loose arrays -------------------------------------------------------------------------
 * For one position j of one kv head, x = the 128 values of the row in the library's element type (K after RoPE, V as is), read as fp32:
 *     amax   = max |x_d|
 *     s      = amax > 0 ? amax / 448 : 1        (fp32 division)  -> scale[j]
 *     inv    = amax > 0 ? 448 / amax : 1        (fp32 division)
 *     byte_d = e4m3fn(clamp(x_d * inv, -448, 448))               round to nearest even; OCP e4m3fn, not fnuz
 * (the rule of trace_op_quant_rows_fp8 on a 128-wide row).  Dequantised value = s * e4m3(byte): 264 bytes per position and kv head instead of 512.
 * Arrays, per layer:
 *     K8     [slot][kvh][ctx][128]          bytes
 *     V8     [slot][kvh][ctx / 32][128][32] bytes: position-blocked V^T, value d of position p is byte (d, p % 32) of the 4 KB block p / 32
 *     ks, vs [slot][kvh][ctx]               fp32
 * The attention widens the bytes to the element type in registers (exact for every finite e4m3 value, bf16 and fp16) and keeps the 16-bit matrix
 * instructions; q and the probabilities are never narrowed.  The scales fold into the per-position scalars:
 *     score_j = (acc_j * scale) * ks[j]         acc = fp32 sum of q . widen(K8[j])
 *     p_j     = exp(score_j - m);  l += p_j     (l sums the unscaled p)
 *     P_j     = round16(p_j * vs[j])            operand of the PV product against widen(V8)
 *     o       = round16((sum_j P_j . widen(V8[j])) / l)
 * Positions past pos[b] inside a 32-position block are read, masked and weigh exactly 0: they must hold finite bytes (not 0x7F / 0xFF) and finite
 * scales (zero-filled arrays do).  trace_amd/kv8.py restates the format in torch.
 * A context keeps its cache in this format under trace_ctx_create_opts(kv_cache_fp8 = 1); the entry points below run the kernels over loose arrays. */
/* trace_op_attn_decode over kv8 arrays (row b in slot b; max_ctx % 32 == 0, nq == 4 nkv, nkv <= 64): q [B][nq * 128] rotated, pos[b] = the newest
 * position, already in the arrays -> O [B][nq * 128]; ws: B * nq * nsplit * 130 floats.  TRACE_ERR_ARG before any launch: B above trace_op_sk_rows(), a
 * shape outside the above, a position outside [0, max_ctx). */
int trace_op_attn_decode_kv8(const void* q, const void* k8, const void* v8, const float* ks, const float* vs, const int32_t* pos, void* O, float* ws,
                             int B, int nq, int nkv, int max_ctx, int nsplit, float scale, void* stream);
/* trace_op_qkv_finish for kv8 arrays: the same sums (chunk order), rounding to the element type and RoPE; the roped q heads go to q_out as there; the
 * new k row and v column of row b are quantised by the rule above and stored at position pos[b] of slot slots[b] — 128 + 128 bytes and the two scales
 * per kv head, nothing else.  Errors as trace_op_qkv_finish. */
int trace_op_qkv_finish_kv8(const float* part, int ks_chunks, void* q_out, void* k8, void* v8, float* ks, float* vs, const int32_t* slots,
                            const int32_t* pos, const float* cos_t, const float* sin_t, int B, int nq, int nkv, int num_slots, int max_ctx, void* stream);
/* 16-bit rows -> kv8: k_rows (roped) / v_rows [B][nkv][R][128], both row-major, become positions pos0 .. pos0 + R - 1 of slot slots[b] (int32 [B]
 * device); nothing outside those positions is written.  TRACE_ERR_ARG before any launch: B above trace_op_sk_rows(), a slot outside [0, num_slots) or
 * given twice, rows outside [0, max_ctx), max_ctx % 32. */
int trace_op_kv8_pack(const void* k_rows, const void* v_rows, void* k8, void* v8, float* ks, float* vs, const int32_t* slots, int pos0, int R, int B,
                      int nkv, int num_slots, int max_ctx, void* stream);
/* kv8 -> 16-bit: positions 0 .. R - 1 of slot slots[b] as round16(s * e4m3) into row b of k_out [B][nkv][max_ctx][128] / vt_out [B][nkv][128][max_ctx]
 * (the 16-bit cache's layout); positions from R on are not written.  Errors as above. */
int trace_op_kv8_unpack(const void* k8, const void* v8, const float* ks, const float* vs, const int32_t* slots, void* k_out, void* vt_out, int R, int B,
                        int nkv, int num_slots, int max_ctx, void* stream);

/* ---- the prefill's cache-write kernels, each alone (tests/test_gpu_prefill_glue_probes.py) ----
 * Pass-throughs of the launchers the prefill calls, with every stride and offset they take.  Each also takes the ELEMENT COUNT of every array the launch
 * will touch and answers TRACE_ERR_ARG, before any launch, when a read or a store would leave one of them, when a pointer is not 16-byte aligned or a
 * stride is no multiple of 8 elements.
 *
 * trace_op_rope_kv: qkv rows [q heads | k heads | v heads] of hd elements, row stride ld >= (nq + 2 nkv) hd.  Row r has
 *   sq = seq_len > 0 ? r / seq_len : 0,  pos = pos_arr ? pos_arr[r] : pos0 + r - sq seq_len,  slot = slot_arr ? slot_arr[r] : slot0 + sq
 * (slot_arr / pos_arr: device int32 [arr_len >= R], either may be NULL).  q heads are rotated in place (rotate-half: the partner of d is d + hd/2;
 * o1 = x1 c - x2 s, o2 = x2 c + x1 s with c, s = cos_t / sin_t [table_rows][hd/2] fp32 at row pos, rounded once); k head h is rotated and stored at
 * kcache[slot slot_stride + h kv_head_stride + pos hd]; with vcache != NULL v head h is copied to the same offset of vcache; nothing else is written.
 * Refused: hd % 16, ld % 8 or below the row width, R / nq / nkv < 1, qkv_elems below (R - 1) ld + width, a position outside 0 .. table_rows - 1, a negative
 * slot, a cache row that ends past kcache_elems (vcache_elems), a position past kv_head_stride with nkv > 1, two rows that go to one cache row. */
int trace_op_rope_kv(void* qkv, int64_t qkv_elems, int ld, void* kcache, int64_t kcache_elems, void* vcache, int64_t vcache_elems, int64_t slot_stride,
                     int64_t kv_head_stride, const int32_t* slot_arr, const int32_t* pos_arr, int64_t arr_len, int slot0, int pos0, int R, int nq, int nkv, int hd,
                     const float* cos_t, const float* sin_t, int table_rows, int seq_len, void* stream);
/* trace_op_transpose_v: dst[b dst_bs + h dst_hs + d dst_rs + p0 + r] = src[b src_bs + h src_hs + r src_rs + d] for r < n, d < hd; positions p0 + n .. the end
 * of that 64-position block become zero, positions below p0 and from that block's end on keep what they hold.  perm = 1 (p0 = 0 only): within every 16
 * positions the stored order is [0-3, 8-11, 4-7, 12-15].  Refused: hd outside {64, 128}, perm outside {0, 1}, perm with p0 != 0, dst_rs % 64,
 * p0 + n > dst_rs, n < 1, p0 < 0, src_rs < hd, heads / batch outside 1..65535, a source or destination the counts cannot hold. */
int trace_op_transpose_v(const void* src, int64_t src_elems, int64_t src_bs, int64_t src_hs, int src_rs, void* dst, int64_t dst_elems, int64_t dst_bs,
                         int64_t dst_hs, int dst_rs, int n, int hd, int heads, int batch, int perm, int p0, void* stream);
/* trace_op_gather_rows: out[r][0 .. H) = tabs[kind[r]][row[r]][0 .. H) for r < L.  tabs: HOST array of six device pointers (NULL = unused), tab_rows: HOST
 * array of their row counts; kind / row: device int32.  Refused: H % 8, L < 1, kind_len or row_len below L, out_elems below L H, a kind outside 0..5, a row
 * outside 0 .. tab_rows[kind] - 1 (so every kind used names a table). */
int trace_op_gather_rows(const void* const* tabs, const int64_t* tab_rows, const int32_t* kind, int64_t kind_len, const int32_t* row, int64_t row_len, void* out,
                         int64_t out_elems, int L, int H, void* stream);


/* ---- The 4-bit weight format ("w4"), and its kernels over loose arrays ----------------------------------------------------------------------------
 * For the four decoder projections W [N][K] (nn.Linear layout, bf16), K % 32 == 0.  A block is 32 consecutive k of one output row.
 *     element  OCP e2m1: magnitudes {0, 0.5, 1, 1.5, 2, 3, 4, 6} = codes 0..7, bit 3 = sign
 *     scale    2^e, one e8m0 byte per block: byte = e + 127
 *     e        the smallest integer with amax / 2^e <= 6 (amax = the block's largest magnitude), so nothing saturates; kept >= -120, so that every
 *              quotient below is a normal fp32 number (bf16 denormals round to code 0).  An all-zero block: every code 0 and byte 0 (e = -127)
 *     code     round to nearest, ties to the even code, of |v| / 2^e (exact: a power-of-two quotient); the sign bit is set only beside a non-zero
 *              magnitude (no negative zeros)
 *     W~[n][k] = e2m1(code) * 2^e — exactly a bf16 value.  Quantising W~ again gives W~ again (possibly under a smaller scale, where a block's largest
 *              code rounded down to 3 or below).
 * Powers of two because the conversion instruction (v_cvt_scalef32_pk_bf16_fp4) is only relied on for power-of-two scale operands.
 * Logical arrays (trace_op_quant_rows_w4, trace_amd/w4.py quant):
 *     codes [N][K / 2]   bytes: k = 2 j in the LOW nibble of byte j, k = 2 j + 1 in the high nibble
 *     exps  [N][K / 32]  bytes
 * Decode tile layout (trace_op_tile_pack_w4, trace_amd/w4.py tile_pack; N % 16 == 0, K % 256 == 0), U = K / 256 units per 16-row tile:
 *     tcodes [N / 16][U][64 lanes][32] bytes: lane = g * 16 + r holds the 64 codes of row tile * 16 + r, k = unit * 256 + g * 64 .. + 64, in logical
 *            byte and nibble order: dword q (0..7) of the 32 bytes is one 8-k matrix fragment, and the conversion instruction takes byte_sel's
 *            low nibble to the low half of its result (tests/test_gpu_w4.py pointer probe)
 *     texps  [N / 16][U][64 lanes][2]  bytes: the exponent bytes of the lane's two blocks (dwords 0-3, dwords 4-7)
 * trace_op_dequant_w4: the tile layout -> row-major bf16 [N][K] = W~, exact.  trace_op_skinny_w4: X bf16 [B][K] . W~^T as fp32 k-chunk partial rows
 * out [KS][trace_op_sk_rows()][N] (KS = out[0] of trace_op_skinny_w4_plan; rows >= B of every chunk are not written), fp32 accumulation of exact
 * bf16 x bf16 products on the bf16 matrix instruction; the caller sums the chunks.  All four: bf16 library only (TRACE_ERR_ARG in the fp16 one). */
int trace_op_quant_rows_w4(const void* W, void* codes, void* exps, int N, int K, void* stream);
int trace_op_tile_pack_w4(const void* codes, const void* exps, void* tcodes, void* texps, int N, int K, void* stream);
int trace_op_dequant_w4(const void* tcodes, const void* texps, void* out, int N, int K, void* stream);
int trace_op_skinny_w4(const void* X, const void* tcodes, const void* texps, float* out, int B, int N, int K, void* stream);

#ifdef __cplusplus
}
#endif
#endif
