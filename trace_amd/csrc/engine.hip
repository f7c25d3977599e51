// Engine behind include/trace_hip.h: owns weights (repacked for the kernels), KV cache and workspaces, and
// sequences the HIP kernels for the three phases of the path
//   video encode (CLIP ViT -> SpatialSlotPool -> [slots | time tokens])  -> splice -> Mistral prefill
//   -> on-device greedy decode with head switching (hipGraph-replayed step, no host round trip per token).
// One context per process / GPU; videos are independent, so multi-GPU is one context per rank (trace_amd/dist.py).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/trace_hip.h"
#include "common.h"
#include "constrain.h"
#include "kernels.h"
#include "logits.h"
#include "sample.h"

static thread_local std::string g_err;
static int fail(int code, const std::string& m) { g_err = m; return code; }
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(TRACE_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)
#define LCHK(x) do { int r_ = (x); if (r_ != TRACE_OK) return fail(r_, std::string("launch failed: ") + #x); } while (0)
#define TRY(x) do { int r_ = (x); if (r_ != TRACE_OK) { if (g_err.empty()) g_err = std::string("failed: ") + #x; return r_; } } while (0)

struct VitLayer {
    bf16_t *ln1w, *ln1b, *wqkv, *bqkv, *wo, *bo, *ln2w, *ln2b, *w1, *b1, *w2, *b2;
};
struct LlmLayer {
    bf16_t *rms1, *wqkv, *wo, *rms2, *wgu, *wd;
    bf16_t *wqkv_d, *wo_d, *wgu_d, *wd_d;      // decode copies in the GEMV tile layout (decode.hip: launch_tile_pack)
    // fp8 weight path (trace_config::llm_weights_fp8; fp8.hip): e4m3 row-major copies for the prefill GEMMs, tile-layout copies for the
    // decode GEMVs, one fp32 scale per output row
    uint8_t *wqkv8, *wo8, *wgu8, *wd8, *wqkv8_d, *wo8_d, *wgu8_d, *wd8_d;
    float *sqkv, *so, *sgu, *sd;
    // w4 weight path (trace_ctx_opts_w4::llm_weights_w4; w4.hip): the ONLY copy of qkv, o, gate|up, down (in this order): e2m1 codes and exponent bytes
    // in the decode tile layout; the 16-bit pointers above stay null
    uint8_t *w4c[4], *w4e[4];
};
// A layer's four projections as a table, in w4c's order (0 qkv, 1 o, 2 gate|up, 3 down): W[N][K] in every copy a body may run it on.
struct Proj {
    int N, K;
    const bf16_t *w, *wd;            // 16-bit: row-major (prefill GEMMs, the wide decode step), GEMV tile layout
    const uint8_t *w8, *w8d;         // e4m3: row-major, tile layout
    const float* sw;                 // their scale per output row
    const uint8_t *w4c, *w4e;        // w4: codes and exponent bytes, tile layout
};
static std::array<Proj, 4> layer_projs(const LlmLayer& W, int H, int I, int QKV) {
    return {{{QKV, H, W.wqkv, W.wqkv_d, W.wqkv8, W.wqkv8_d, W.sqkv, W.w4c[0], W.w4e[0]}, {H, H, W.wo, W.wo_d, W.wo8, W.wo8_d, W.so, W.w4c[1], W.w4e[1]},
             {2 * I, H, W.wgu, W.wgu_d, W.wgu8, W.wgu8_d, W.sgu, W.w4c[2], W.w4e[2]}, {H, I, W.wd, W.wd_d, W.wd8, W.wd8_d, W.sd, W.w4c[3], W.w4e[3]}}};
}
struct StcBlock { bf16_t *w1, *n1w, *n1b, *wdw, *n2w, *n2b, *fc1w, *fc1b, *fc2w, *fc2b, *w3, *n3w, *n3b, *wd, *ndw, *ndb; int cin, rd; };

constexpr int PF_MAX = 4;        // equal-length prompts of max_ctx rows one prefill pass can take: the workspaces hold pf_rows() rows, and a pass takes up to PF_MAX_N
constexpr int PF_MAX_N = 8;      // SHORTER prompts while n x L fits them (round 6: four 1086-row Charades prompts are 17 row panels = 1.06 rounds of the o / down tile grid)
static size_t pf_rows(int max_ctx) { return std::max<size_t>((size_t)PF_MAX * max_ctx, std::min<size_t>(8192, (size_t)PF_MAX_N * max_ctx)); }
constexpr int MAX_SLOTS = 512;   // KV-cache sequence slots per context (a decode batch is at most SK_ROWS of them)
static int g_ctx_per_dev[16] = {0};
// what the tail of a decode step does beyond the plain arg-max; index(): its place in the graph cache, 0 = the plain step
// per_row: the batch carries per-row generation parameters (trace_decode_set_row_params) — places 16 .. 31, which no batch without them ever takes
struct TailMode {
    bool sample = false, logprobs = false, process = false, stop = false, per_row = false;
    int index() const { return (sample ? 1 : 0) + (logprobs ? 2 : 0) + (process ? 4 : 0) + (stop ? 8 : 0) + (per_row ? 16 : 0); }
};
constexpr int TAIL_MODES = 32;
static_assert(sizeof(SampleParams) == 4 * retire_rowp_ints(0) && sizeof(LogitsParams) == 4 * retire_rowp_ints(1), "retire.hip moves the per-row params as ints");

static bool constraints_on(const ConstrainTable& t) { return t.n_stop || t.n_bad || t.n_suppress || t.n_begin; }

struct trace_ctx {
    trace_config c{};
    int dev = 0;
    // derived
    int H, I, NL, NQ, NKV, HD, V, Tv, Sv, NV, NVpad, QKV;
    int vh, vi, vL, vheads, G, GG, NT, P, Kpatch, Kpad, tokpad;
    int S, TPF;                      // slots per frame, tokens per frame (slots + 6)
    int max_ctx, max_B, ctx_pad;
    int vit_frames;                  // frames one trace_vit_forward call may take (>= max_frames)
    std::vector<void*> allocs;
    size_t total_bytes = 0;
    std::unordered_map<std::string, int> loaded;
    bool finalized = false;
    bool counted = false;            // in g_ctx_per_dev (the last context of a device frees the persistent GEMM's ticket counters)
    // weights
    bf16_t *patch_w, *cls, *pos_emb, *pre_w, *pre_b;
    bf16_t *patch_wp = nullptr, *cls_row = nullptr;      // fused patch embedding (patch_embed.hip): repacked conv weight, the CLS row
    std::vector<VitLayer> vit;
    bf16_t *sl_lnw, *sl_lnb, *sl_slots, *sl_readout;
    // STC connector (projector_type == 1)
    int stc = 0, stc_loaded = 0;
    StcBlock stc_blk[2][4];
    bf16_t *stc_w3d, *stc_b3d, *stc_r0w, *stc_r0b, *stc_r2w, *stc_r2b;
    bf16_t *stc_x, *stc_y, *stc_z, *stc_sc, *stc_col, *stc_pool, *stc_g1, *stc_g2, *stc_tmp;
    bf16_t *embed, *final_norm, *wheads, *time_tab, *score_tab, *sync_row;
    std::vector<LlmLayer> llm;
    float *slot_cos, *slot_sin, *rope_cos, *rope_sin;
    // KV cache: K [layer][slot][kvh][ctx_pad][hd] row-major; V TRANSPOSED [layer][slot][kvh][hd][ctx_pad] (decode.hip)
    bf16_t *kcache, *vcache;
    size_t kv_head_stride, slot_stride, layer_stride;
    // e4m3 KV cache (trace_ctx_create_opts, kv8.hip): K8 / V8 bytes [layer][slot][kvh][...] with the strides above in BYTES, ks / vs fp32 with those / HD,
    // instead of kcache / vcache; kv_stage_k / kv_stage_v = ONE layer's 16-bit K / V^T of PF_MAX_N slots (the strides above in elements) that every layer's
    // prefill attention runs on before its rows are packed; d_ident = 0 .. MAX_SLOTS - 1 (slot lists of the pack / unpack launches)
    int kv8 = 0;
    uint8_t *k8cache = nullptr, *v8cache = nullptr;
    float *kscache = nullptr, *vscache = nullptr;
    bf16_t *kv_stage_k = nullptr, *kv_stage_v = nullptr;
    int32_t* d_ident = nullptr;
    // ViT workspaces
    bf16_t *vX, *vH, *vQKV, *vVT, *vMLP;
    bf16_t *sl_res, *sl_out, *video;     // [T*S, vh], [T*S, H], [T*TPF, H]
    float* sl_ws = nullptr; size_t sl_ws_floats = 0;   // slot pool: per-part softmax partials
    int video_rows = 0;
    // LLM prefill workspaces
    bf16_t *pX, *pH, *pQKV, *pO, *pACT;
    int32_t *d_kind, *d_row;             // splice index arrays (max_ctx)
    int32_t *h_kind, *h_row;             // pinned host staging: the buffer of the ring below that the current call fills
    static constexpr int NSTAGE_H = 4;   // ring of staging buffers, each behind an event recorded after its last copy was queued (round 6: the two calls that use
    int32_t* h_ring = nullptr;           // them waited for the whole stream instead — two drains of the encode stream per video)
    hipEvent_t h_ev[NSTAGE_H] = {nullptr, nullptr, nullptr, nullptr};
    int h_next = 0; size_t h_len = 0;
    int spliced_len = 0;
    // decode state
    bf16_t *dX, *dH, *dQKV, *dO, *dACT, *xlast;   // [SK_ROWS, *]: one row per sequence of the decode batch; xlast [slots, H]: every KV slot's last prefill hidden row
    float* attn_ws; unsigned int* tickets;
    void* pp_buf = nullptr; size_t pp_bytes = 0;       // frame preprocessing: tap tables + staged rows (grow-only)
    float* sk_ws = nullptr; unsigned int* sk_tickets = nullptr; size_t sk_ws_floats = 0; int sk_ntickets = 0;   // decode GEMV K-chunk partials
    float* sk_ws2 = nullptr;           // second partial-row buffer and residual rows: the fused-norm GEMVs of small batches read one and write the other
    bf16_t* dX2 = nullptr;
    float* part_val; int32_t* part_idx;
    float* hl_val; int32_t* hl_idx;        // trace_llm_head_logits' own partial buffers
    int32_t *d_slots, *d_pos, *d_heads, *d_done, *d_out_ids, *d_out_len, *d_step, *d_forced, *d_params;
    int32_t* d_row_id = nullptr;       // [SK_ROWS] Philox row index of every row of the batch: identity at trace_decode_begin, gathered by trace_decode_retire
    int32_t* d_step0 = nullptr;        // [SK_ROWS] the value of d_step[0] at which each row's own step 0 happened: zeros at trace_decode_begin, set by trace_decode_admit,
                                       // gathered by trace_decode_retire.  Always passed (never null): a step graph captured before an admission reads the same array after it
    int32_t h_step0[SK_ROWS] = {0};    // host copy of d_step0 (trace_decode_steps' per-row bound)
    int32_t h_slots[SK_ROWS] = {0};    // host copy of d_slots (trace_decode_admit refuses a slot the batch holds)
    int admitted = 0;                  // rows admitted since trace_decode_begin
    int32_t* d_retire = nullptr;       // trace_decode_retire's keep list [SK_ROWS] and scratch rows (allocated at the first retire)
    int32_t h_pos0[SK_ROWS] = {0};     // host copy: the prefill length of every row of the batch (pos_sum after a retire)
    int32_t* d_heads_tmp;                // head id per row for trace_llm_head_logits
    int B = 0, max_new = 0, eos = -1, ntiles = 0, nsplit = 32;
    int slot_len[MAX_SLOTS] = {0};
    int fp8 = 0;                       // decoder projections on the fp8 path
    int fp8_wonly = 0;                 // llm_weights_fp8 == 2: the decode GEMVs keep bf16 activations (weight-only; the prefill GEMMs stay W8A8)
    uint8_t *pA8 = nullptr, *dA8 = nullptr, *dH8 = nullptr;      // quantised activations: prefill [2 max_ctx][max(H, I)], decode [64][I]; dH8 = the normed hidden rows
    float *psa = nullptr, *dsa = nullptr, *dsh = nullptr;        // their per-row scales
    // w4 weights: one layer's 16-bit row-major qkv, o, gate|up, down that dequant_w4 fills before each prefill layer (and that a tensor lands in while it
    // is loaded), and the logical codes / exponents of one loaded piece between the quantiser and the tile packer
    int w4 = 0;
    bf16_t* w4_row[4] = {nullptr, nullptr, nullptr, nullptr};
    uint8_t *w4_stage_c = nullptr, *w4_stage_e = nullptr;
    int step_in_call = 0;              // decode steps taken since trace_decode_begin at the time decode_step runs (host copy)
    long pos_sum = 0;                  // sum over the batch of the prefill lengths (host copy: algorithmic KV bytes of a decode step's attention)
    double kbytes_sum = 0.0;           // algorithmic bytes of the bracketed launches (profile == 2)
    int host_mode = 0, fed = 0;        // host-driven token selection (sampling): head logits only, ids fed back by the host
    int steps_done = 0;                // decode steps taken since trace_decode_begin (bounded by max_new - 1: the KV slot and the RoPE tables end at max_ctx)
    // What the tail of a step (head_and_select) does beyond the plain arg-max: `want` is written by the four trace_decode_set_* calls, `armed` at
    // trace_decode_begin (= want, or all-off in host-select mode, where the host holds the logits and does all of it itself).  A step of each
    // mode is a graph of its own, graphs[armed.index()][B]: toggling a setting between batches never replays another form, and index 0 is the plain step.
    TailMode want, armed;
    // Shared prompt prefix of the batch being decoded (trace_decode_set_shared_prefix): the decode attention reads positions below sh_rows (a multiple of
    // 32, 0 = off) of every sequence from slot sh_slot.  sh_want_* is the request the next trace_decode_begin consumes.  Both are launch arguments of the
    // attention, so a captured step is good for one (slot, rows) pair: a graph entry has two ways keyed by it (the two banks of a pipelined caller).
    int sh_want_slot = -1, sh_want_rows = 0, sh_slot = -1, sh_rows = 0;
    struct StepGraph { hipGraphExec_t exec = nullptr; int sh_slot = -1, sh_rows = 0; };
    StepGraph graphs[TAIL_MODES][SK_ROWS + 1][2];
    int graph_evict = 0;               // the way the next miss of a full entry replaces
    // sampling (trace_decode_set_sampling): host copy of the params; the device copy d_sparams, written at trace_decode_begin, is what the selection
    // kernel reads (a captured graph stays valid across calls).  d_slog: the [SK_ROWS][NV] raw masked logits of a step with anything armed.
    SampleParams samp{};
    SampleParams* d_sparams = nullptr;
    float* d_slog = nullptr;
    // per-token log-probabilities (trace_decode_set_logprobs): d_logprobs [SK_ROWS][max_new_tokens] (rows of the current batch at stride max_new),
    // written by the launch after the selection from the d_slog rows
    float* d_logprobs = nullptr;
    // scoring given tokens (trace_llm_score_rows / _append, score.hip): allocated on first use for pf_rows() rows — the tile partials, the rows' heads
    // and target ids, their log-probabilities
    float* score_ws = nullptr; int32_t* d_score_heads = nullptr; int32_t* d_score_ids = nullptr; float* d_score_out = nullptr;
    // logits processors (trace_decode_set_logits_params): the device copy d_lgparams, written at trace_decode_begin, is what logits_process_kernel
    // reads, d_plog the [SK_ROWS][NV] processed rows the selection then reads (d_slog stays raw: the log-probabilities' rows)
    LogitsParams lgp{1.f, 0, 0};
    LogitsParams* d_lgparams = nullptr;
    float* d_plog = nullptr;
    // per-row generation parameters (trace_decode_set_row_params, trace_decode_admit_ex): three arrays of SK_ROWS entries beside d_row_id / d_step0 that
    // the tail of a batch begun with them reads instead of d_sparams / d_lgparams / d_params[0] (StepState::row_sp / row_lp / row_max_new); they move
    // with the row (trace_decode_retire) and keep their addresses, which the captured steps hold.  h_row_*: the host copies (the bounds of
    // trace_decode_steps, the decision whether logits_process runs); want_rows: the request the next trace_decode_begin consumes.
    SampleParams* d_row_sp = nullptr;
    LogitsParams* d_row_lp = nullptr;
    int32_t* d_row_max = nullptr;
    SampleParams h_row_sp[SK_ROWS];
    LogitsParams h_row_lp[SK_ROWS];
    int32_t h_row_max[SK_ROWS] = {0};
    std::vector<trace_row_params> want_rows;
    // constraints (trace_decode_set_constraints, constrain.h): the host copy of the table; the device copy d_ctab, written at trace_decode_begin, is what
    // logits_process_kernel (the ban rules: want.process is "any logits param or any ban rule") and select_next_kernel (want.stop) read.  It exists from
    // the first arming of either, so a captured step of either kind always holds its address.
    ConstrainTable ctab{};
    ConstrainTable* d_ctab = nullptr;
    hipStream_t cap_stream = nullptr;
    std::vector<hipStream_t> streams;   // trace_stream_create
    // profiling
    int profile = 0;                  // 1: time decode_steps calls; 2: also bracket the layer-0 gate|up GEMV launch
    int bracket_mask = 3;             // which per-launch brackets profile == 2 takes: bit 0 = the ViT fc1 GEMM, bit 1 = the decode step's kernel; instead of
                                      // bit 1, bit 2 = the layer-0 decode attention of every step body, bit 3 = the layer-0 append launch (qkv_finish)
                                      // (trace_set_profile_brackets: a pipelined caller switches a stage's bracket off while the other stage's
                                      // kernels share the GPU with it — an event pair then times the queueing, not the kernel)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<hipEvent_t> kev;      // event pool for per-launch brackets (eager mode)
    int kev_used = 0;
    double ksum_ms = 0.0; int ksamples = 0;
    hipEvent_t mev0 = nullptr, mev1 = nullptr;   // bracket of one ViT fc1 GEMM launch per trace_vit_forward (profile == 2)
    double msum_ms = 0.0; int msamples = 0; double mflops = 0.0; int mM = 0;
    // the other three GEMM shapes of the layer (qkv, out-proj, fc2), bracketed the same way in layer 0: the 256x256 MFMA GEMM family is the run's
    // dominant kernel and its four shapes sit at different fractions of the peak — the line reports each (pairs 0 = qkv, 1 = out-proj, 2 = fc2)
    hipEvent_t vev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    double vsum_ms[3] = {0.0, 0.0, 0.0}; double vflops[3] = {0.0, 0.0, 0.0};
    float prof[20] = {0};
    int bracket_kind = 0;             // which launch the decode bracket of profile == 2 was put around: 0 none yet, 1 = gate|up GEMV (skinny path), 2 = the fused-norm
                                      // gate|up GEMV of a batch-1 step, 3 = the layer-0 decode attention, 4 = the layer-0 append launch
};

template <typename T>
static int dalloc(trace_ctx* c, T** p, size_t n_elems) {
    void* q = nullptr;
    const size_t bytes = (n_elems * sizeof(T) + 255) & ~(size_t)255;
    HIPCHK(hipMalloc(&q, bytes));
    HIPCHK(hipMemset(q, 0, bytes));
    c->allocs.push_back(q);
    c->total_bytes += bytes;
    *p = (T*)q;
    return TRACE_OK;
}

#define SKWS(c) (c)->sk_ws, (c)->sk_ws_floats, (c)->sk_tickets, (c)->sk_ntickets
static int round_up(int x, int m) { return (x + m - 1) / m * m; }

extern "C" const char* trace_last_error(void) { return g_err.c_str(); }

// ------------------------------------------------------------------------------------------------ tuning table (tuning.h)
// One row per field of Tuning: its dotted name, the values trace_op_tuning_set accepts, the default, what it does (and the measurements behind it).
struct TuneRow { const char* name; int Tuning::*field; int lo, hi, dflt; const char* doc; };
static const TuneRow TUNE_ROWS[] = {
    {"gemm.kernel", &Tuning::gemm_kernel, 0, 8, 0, "0 = auto routing, 2 = 128^2 tiles, 3 = gemm.hip's 256^2 kernel, 4 = loader-wave kernel, 5 / 6 / 7 = persistent kernel ticketed / static deal / one workgroup per tile, 8 = its 4-wave form"},
    {"gemm.w4", &Tuning::gemm_w4, 0, 1, 1, "auto routing: non-residual 256^2 shapes on gemm_w4.hip (1) or gemm_pers.hip (0); TRACE_GEMM_W4 sets the initial value"},
    {"gemm.resid_pers", &Tuning::gemm_resid_pers, 0, 1, 0, "auto routing: 1 = residual shapes run on the persistent kernel too"},
    {"gemm.pers.walk", &Tuning::gemm_pers_walk, 0, 1, 0, "tile walk of every persistent route: 0 = tickets with atomic re-arm, 1 = static deal"},
    {"gemm.pers.opt", &Tuning::gemm_pers_opt, 0, 63, 0, "A/B builds of the gemm_pers.hip K loop (2, 4, 8; anything else = the shipped one)"},
    {"gemm.pers.grid_cap", &Tuning::gemm_pers_grid_cap, 0, 1024, 0, "at most this many workgroups per persistent launch (0 = #CUs); a stream's own cap (trace_set_gemm_cus) comes first"},
    {"gemm.ldr.opt", &Tuning::gemm_ldr_opt, 0, 3, 0, "gemm_ldr.hip: bit 0 = no residual touches, bit 1 = no A-panel touches"},
    {"gemm.w4.opt", &Tuning::gemm_w4_opt, 0, 7, 0, "gemm_w4.hip: bit 0 = without the re-aligning barrier, bit 2 = with the L2 touches of the A panel; 2 = the check build (vmcnt(0) waits)"},
    {"decode.wide_min_rows", &Tuning::decode_wide_min_rows, 17, 65, 32, "smallest batch that takes the wide (GEMM) decode step (65 = only above the GEMV's 64 rows) — ms per step, GEMV path vs wide step (r03_decode_gemm_ab.txt): 32 rows 5.39 / 5.30, 48 rows 7.19 / 6.51, 64 rows 7.88 / 7.11"},
    {"decode.wide_fuse_qkv", &Tuning::decode_wide_fuse_qkv, 0, 1, 0, "wide decode step: 1 = the attention's fused prologue sums the qkv partial rows, applies RoPE and appends k / v itself (no qkv_finish launch; same sums and roundings, bit-identical)"},
    {"decode.gemm_tiled", &Tuning::decode_gemm_tiled, 0, 31, 21, "wide decode step, GemmArgs::w_tiled: bit 0 = weights from the decode tile copies (0 = row-major prefill copies), bit 2 = 4-stage K-tile ring, bit 4 = partial rows stored write-through (sc1): the consumer's kernel boundary has no dirty partial bytes to write back (round 6, same bits: 10.41 -> 10.33 ms per 128-sequence step; bit 1 = nt weight DMA +2.7 %, bit 3 = nt partial stores +0.4 %: off)"},
    {"decode.fuse_norm_rows", &Tuning::decode_fuse_norm_rows, 0, 4, 1, "batches up to this size take decode_step_fused (0 = never).  Measured, ms per step, unfused / fused (profiles/r03_decode_small_ab.txt): batch 1 3.596 / 3.531, batch 2 3.698 / 3.781, batch 4 3.888 / 4.327 — every workgroup redoes the row sums, which only a single row repays"},
    {"decode.fuse_swiglu", &Tuning::decode_fuse_swiglu, 0, 1, 1, "decode_step_fused: SwiGLU inside the down GEMV (bit-identical to swiglu_combine + GEMV)"},
    {"decode.unfused_qkv", &Tuning::decode_unfused_qkv, 0, 2, 0, "RoPE + cache append as a kernel of its own before the decode attention: 0 = from batch 32 up (bit-identical to the fused prologue, 1 % faster per 64-sequence step, one launch more — which batch 1 would feel), 1 = always, 2 = never (tools/decode_variant_ab.py --variants 122,121)"},
    {"decode.partial_cfg", &Tuning::decode_partial_cfg, 0, 3, 0, "tile of the decode partial-row GEMM: 0 = 128 x 128 on 2 x 2 waves, 1 / 2 / 3 = 128 x 64 on 4 x 1 waves with a 5- / 3- / 4-stage ring"},
    {"decode.partial_wgs", &Tuning::decode_partial_wgs, 0, 1024, 192, "workgroup target of gemm_partial_ks (0 = the initial value); TRACE_PARTIAL_WGS sets the initial value"},
    {"attn.decode.debug", &Tuning::attn_decode_debug, 0, 9, 0, "microbenchmark-only phase cut-offs of the decode attention (0 = full kernel; 8: V^T read as contiguous blocks, timing only)"},
    {"attn.decode.waves", &Tuning::attn_decode_waves, -1, 4, -1, "waves per decode-attention workgroup: -1 / 0 / 2 = 4 (ships), 1 = 3, 3 = 6, 4 = 8"},
    {"attn.decode.nt", &Tuning::attn_decode_nt, 0, 1, 0, "non-temporal cache loads in the decode attention"},
    {"attn.decode.lds_pad_kb", &Tuning::attn_decode_lds_pad_kb, 0, 152, 0, "KB of unused dynamic LDS per decode-attention workgroup (caps the workgroups per CU)"},
    {"attn.decode.nsplit", &Tuning::attn_decode_nsplit, 0, 16, 0, "context splits of the decode attention forced to this number (0 = decode_route's rule)"},
    {"attn.prefill.debug", &Tuning::attn_prefill_debug, 0, 9, 0, "microbenchmark-only knock-outs of the prefill-shaped kernels: 1 = no K/V loads after tile 0, 2 = no tile math, 5 = no LDS-DMA ViT kernel, 6 = its transposed-V path"},
    {"attn.vit.big", &Tuning::attn_vit_big, 0, 2, 2, "ViT attention: 0 = the 4 x 32-row kernel, 1 = the 192-row kernel with a 4-stage ring, 2 = with a 3-stage ring"},
    {"skinny.debug", &Tuning::skinny_debug, 0, 9, 0, "microbenchmark-only, decode GEMV: 3 = stop before the epilogue, 4 = stop after the partial stores (ticket path)"},
    {"prefill.last_rows", &Tuning::prefill_last_rows, 0, 1, 1, "0 = the last decoder layer of a prefill runs over all rows like the others (bit-identical)"},
    {"vit.patch_fused", &Tuning::vit_patch_fused, 0, 1, 1, "0 = im2col matrix -> GEMM -> assemble instead of the fused ViT front end"},
};
const Tuning& tuning_initial() {
    static const Tuning init = [] {
        Tuning t{};
        for (const TuneRow& r : TUNE_ROWS) t.*r.field = r.dflt;
        if (const char* e = getenv("TRACE_GEMM_W4")) t.gemm_w4 = atoi(e) != 0;
        if (const char* e = getenv("TRACE_PARTIAL_WGS")) t.decode_partial_wgs = atoi(e);
        return t;
    }();
    return init;
}
Tuning g_tune = tuning_initial();

static int tune_row(const char* name, const TuneRow** row) {
    for (const TuneRow& r : TUNE_ROWS) if (name && !strcmp(name, r.name)) { *row = &r; return TRACE_OK; }
    return fail(TRACE_ERR_ARG, std::string("unknown tuning value: ") + (name ? name : "(null)"));
}
extern "C" int trace_op_tuning_set(const char* name, int value) {
    const TuneRow* r;
    TRY(tune_row(name, &r));
    if (value < r->lo || value > r->hi) return fail(TRACE_ERR_ARG, std::string(r->name) + " must be " + std::to_string(r->lo) + ".." + std::to_string(r->hi));
    g_tune.*r->field = value;
    return TRACE_OK;
}
extern "C" int trace_op_tuning_get(const char* name, int* value) {
    const TuneRow* r;
    if (!value) return fail(TRACE_ERR_ARG, "null pointer");
    TRY(tune_row(name, &r));
    *value = g_tune.*r->field;
    return TRACE_OK;
}
extern "C" int trace_op_tuning_reset(void) { g_tune = tuning_initial(); return TRACE_OK; }
extern "C" const char* trace_op_tuning_name(int i) { return i >= 0 && i < (int)(sizeof(TUNE_ROWS) / sizeof(TUNE_ROWS[0])) ? TUNE_ROWS[i].name : nullptr; }

// The numeric codes of trace_op_set_gemm_variant (bench.py, tools/*, DESIGN.md and the profiles speak in them): code in [lo, hi] stores
// base + (code - lo) * scale.  The only place these numbers live.
struct LegacyCode { int lo, hi; int Tuning::*field; int scale, base; };
static const LegacyCode LEGACY_CODES[] = {
    {0, 8, &Tuning::gemm_kernel, 1, 0},
    {100, 109, &Tuning::attn_decode_debug, 1, 0},
    {110, 119, &Tuning::attn_prefill_debug, 1, 0},
    {120, 122, &Tuning::decode_unfused_qkv, 1, 0},
    {130, 137, &Tuning::decode_gemm_tiled, 1, 0},           // the low three bits of the word 700+ sets
    {140, 140, &Tuning::decode_wide_min_rows, 0, SKINNY_ROWS + 1},
    {141, 141, &Tuning::decode_wide_min_rows, 0, 33},
    {142, 142, &Tuning::decode_wide_min_rows, 0, 17},
    {143, 143, &Tuning::decode_wide_min_rows, 0, 32},
    {144, 145, &Tuning::decode_wide_fuse_qkv, 1, 0},
    {160, 161, &Tuning::vit_patch_fused, 1, 0},
    {170, 174, &Tuning::decode_fuse_norm_rows, 1, 0},
    {180, 181, &Tuning::decode_fuse_swiglu, 1, 0},
    {190, 192, &Tuning::attn_vit_big, 1, 0},
    {200, 209, &Tuning::skinny_debug, 1, 0},
    {300, 363, &Tuning::gemm_pers_opt, 1, 0},
    {400, 403, &Tuning::gemm_ldr_opt, 1, 0},
    {500, 501, &Tuning::gemm_pers_walk, 1, 0},
    {520, 521, &Tuning::gemm_resid_pers, 1, 0},
    {530, 531, &Tuning::gemm_w4, 1, 0},
    {540, 547, &Tuning::gemm_w4_opt, 1, 0},
    {700, 731, &Tuning::decode_gemm_tiled, 1, 0},
    {740, 743, &Tuning::decode_partial_cfg, 1, 0},
    {750, 751, &Tuning::prefill_last_rows, 1, 0},
    {760, 761, &Tuning::attn_decode_waves, 1, 0},
    {762, 762, &Tuning::attn_decode_waves, 0, -1},
    {763, 764, &Tuning::attn_decode_waves, 1, 3},
    {770, 771, &Tuning::attn_decode_nt, 1, 0},
    {780, 799, &Tuning::attn_decode_lds_pad_kb, 8, 0},
    {800, 832, &Tuning::decode_partial_wgs, 32, 0},
    {850, 866, &Tuning::attn_decode_nsplit, 1, 0},
    {1000, 2024, &Tuning::gemm_pers_grid_cap, 1, 0},
};
extern "C" int trace_op_set_gemm_variant(int variant) {
    for (const LegacyCode& r : LEGACY_CODES)
        if (variant >= r.lo && variant <= r.hi) { g_tune.*r.field = r.base + (variant - r.lo) * r.scale; return TRACE_OK; }
    return fail(TRACE_ERR_ARG, "variant must be 0..8");
}
extern "C" int trace_op_gemm_route(int M, int N, int K, int lda, int ldw, int ldc, int ldr, int epilogue, int fp8) {
    GemmArgs g{};
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldw = ldw; g.ldc = ldc; g.ldr = ldr; g.fp8 = fp8;
    if (!gemm_shape_ok(g, epilogue)) return fail(TRACE_ERR_ARG, "launch_gemm_bf16 does not take this shape");
    const GemmRoute r = gemm_route(g, epilogue, g_tune);
    return (int)r.k | r.walk << 8;
}

extern "C" int trace_abi_version(void) { return TRACE_ABI_VERSION; }
extern "C" int trace_element_type(void) { return TRACE_ELEMENT_TYPE; }

static int ctx_create(const trace_config* cfg, int device_id, int kv8, int w4, trace_ctx** out);
extern "C" int trace_ctx_create(const trace_config* cfg, int device_id, trace_ctx** out) { return ctx_create(cfg, device_id, 0, 0, out); }
extern "C" int trace_ctx_create_opts(const trace_config* cfg, int device_id, const trace_ctx_opts* opts, trace_ctx** out) {
    if (!cfg || !out) return fail(TRACE_ERR_ARG, "null argument");
    if (opts && opts->size < (int32_t)sizeof(trace_ctx_opts)) return fail(TRACE_ERR_ARG, "trace_ctx_opts::size is smaller than this library's struct");
    const int kv8 = opts ? opts->kv_cache_fp8 : 0;
    if (kv8 != 0 && kv8 != 1) return fail(TRACE_ERR_ARG, "kv_cache_fp8 must be 0 or 1");
    if (kv8 && cfg->llm_weights_fp8) return fail(TRACE_ERR_ARG, "kv_cache_fp8 with llm_weights_fp8: the e4m3 KV cache runs on 16-bit weights only");
    // the 12-byte form (trace_ctx_opts_w4) carries llm_weights_w4 behind the two fields of the 8-byte one
    const int w4 = opts && opts->size >= (int32_t)sizeof(trace_ctx_opts_w4) ? reinterpret_cast<const trace_ctx_opts_w4*>(opts)->llm_weights_w4 : 0;
    if (w4 != 0 && w4 != 1) return fail(TRACE_ERR_ARG, "llm_weights_w4 must be 0 or 1");
    if (w4 && cfg->llm_weights_fp8) return fail(TRACE_ERR_ARG, "llm_weights_w4 with llm_weights_fp8: the decoder projections take one quantised format");
    if (w4 && kv8) return fail(TRACE_ERR_ARG, "llm_weights_w4 with kv_cache_fp8: the e4m3 KV cache runs on 16-bit weights only");
    if (w4 && TRACE_ELEMENT_TYPE != 0) return fail(TRACE_ERR_ARG, "llm_weights_w4 needs the bf16 library (the fp16 build has no w4 weight path)");
    if (w4 && (cfg->hidden_size % 256 || cfg->intermediate_size % 256)) return fail(TRACE_ERR_ARG, "w4 weight path needs hidden / intermediate sizes that are multiples of 256");
    return ctx_create(cfg, device_id, kv8, w4, out);
}
extern "C" int trace_ctx_kv_cache_type(trace_ctx* c) { return c ? c->kv8 : fail(TRACE_ERR_ARG, "null context"); }
extern "C" int trace_ctx_llm_weights_type(trace_ctx* c) { return c ? (c->w4 ? 3 : c->fp8 ? 1 + c->fp8_wonly : 0) : fail(TRACE_ERR_ARG, "null context"); }
static int ctx_create(const trace_config* cfg, int device_id, int kv8, int w4, trace_ctx** out) {
    if (!cfg || !out) return fail(TRACE_ERR_ARG, "null argument");
    g_err.clear();
    HIPCHK(hipSetDevice(device_id));
    trace_ctx* c = new trace_ctx();
    c->c = *cfg;
    c->dev = device_id;
    c->kv8 = kv8;
    c->w4 = w4;
    c->H = cfg->hidden_size; c->I = cfg->intermediate_size; c->NL = cfg->num_layers;
    c->NQ = cfg->num_heads; c->NKV = cfg->num_kv_heads; c->HD = c->H / c->NQ;
    c->V = cfg->vocab_size; c->Tv = cfg->time_vocab; c->Sv = cfg->score_vocab;
    c->NV = c->V + 1 + c->Tv + c->Sv; c->NVpad = round_up(c->NV, 16);
    c->QKV = (c->NQ + 2 * c->NKV) * c->HD;
    c->vh = cfg->v_hidden; c->vi = cfg->v_inter; c->vL = cfg->v_layers_used; c->vheads = cfg->v_heads;
    c->P = cfg->v_patch; c->G = cfg->v_image / cfg->v_patch; c->GG = c->G * c->G; c->NT = c->GG + 1;
    c->Kpatch = 3 * c->P * c->P; c->Kpad = round_up(c->Kpatch, 64); c->tokpad = round_up(c->NT, 64);
    c->S = cfg->num_slots; c->TPF = c->S + 6;
    c->max_ctx = cfg->max_ctx; c->max_B = cfg->max_batch; c->ctx_pad = round_up(c->max_ctx, 64);
    c->vit_frames = cfg->vit_batch_frames > cfg->max_frames ? cfg->vit_batch_frames : cfg->max_frames;
    auto bad = [&](const char* m) { delete c; return fail(TRACE_ERR_ARG, m); };
    if (c->HD != 128 || c->NQ != 4 * c->NKV) return bad("LLM kernels need head_dim 128 and 4:1 GQA");
    if (c->vh / c->vheads != 64) return bad("ViT kernels need head_dim 64");
    if (c->H % 128 || c->I % 128 || c->vh % 128 || c->vi % 128 || c->QKV % 128) return bad("dims must be multiples of 128");
    if (c->H > 4096) return bad("hidden_size > 4096: the decode row kernels (norms, residual add) hold one 4096-wide row per workgroup");
    c->stc = cfg->projector_type == 1;
    if (cfg->llm_weights_fp8 && TRACE_ELEMENT_TYPE != 0) { delete c; return fail(TRACE_ERR_ARG, "llm_weights_fp8 needs the bf16 library (the fp16 build has no fp8 weight path)"); }
    c->fp8 = cfg->llm_weights_fp8 != 0;
    c->fp8_wonly = cfg->llm_weights_fp8 == 2;
    if (c->fp8 && (c->H % 128 || c->I % 128 || c->I > 16384)) return bad("fp8 weight path needs hidden / intermediate sizes that are multiples of 128 (intermediate <= 16384)");
    if (!c->stc && (c->S != 8 || c->vh > 1024)) return bad("slot pool kernel needs 8 slots and mm_hidden <= 1024");
    if (c->max_B < 1 || c->max_B > MAX_SLOTS) return bad("max_batch (KV slots) must be in [1,512]");
    c->nsplit = 32;                                           // upper bound (workspace size); per-batch value below
    {
        const int g2 = c->G / 2 + 1;
        const int vis_rows = c->stc ? (cfg->max_frames / 2 + 1) * g2 * g2 : cfg->max_frames * c->TPF;
        if (cfg->max_frames < 1 || vis_rows > c->max_ctx) return bad("visual tokens of max_frames exceed max_ctx");
        if (c->stc && cfg->max_frames > 32) return bad("STC connector path supports at most 32 frames");
    }

    const size_t H = c->H, I = c->I, vh = c->vh, vi = c->vi;
    int rc = TRACE_OK;
#define A(p, n) if (rc == TRACE_OK) rc = dalloc(c, &(p), (size_t)(n))
    // --- weights ---
    A(c->patch_w, vh * c->Kpad); A(c->cls, vh); A(c->pos_emb, (size_t)c->NT * vh); A(c->pre_w, vh); A(c->pre_b, vh);
    if (patch_embed_supported(cfg->v_image, c->P, (int)vh)) { A(c->patch_wp, patch_embed_packed_elems(c->P, (int)vh)); A(c->cls_row, vh); }
    c->vit.resize(c->vL);
    for (auto& l : c->vit) {
        A(l.ln1w, vh); A(l.ln1b, vh); A(l.wqkv, 3 * vh * vh); A(l.bqkv, 3 * vh); A(l.wo, vh * vh); A(l.bo, vh);
        A(l.ln2w, vh); A(l.ln2b, vh); A(l.w1, vi * vh); A(l.b1, vi); A(l.w2, vh * vi); A(l.b2, vh);
    }
    if (!c->stc) { A(c->sl_lnw, vh); A(c->sl_lnb, vh); A(c->sl_slots, vh * c->S); A(c->sl_readout, H * vh); }
    else {
        for (int st = 0; st < 2; ++st)
            for (int b = 0; b < 4; ++b) {
                StcBlock& k = c->stc_blk[st][b];
                k.cin = (st == 0 && b == 0) ? (int)vh : (int)H;
                k.rd = (int)lround(k.cin * 0.25);
                A(k.w1, H * k.cin); A(k.n1w, H); A(k.n1b, H); A(k.wdw, H * 9); A(k.n2w, H); A(k.n2b, H);
                A(k.fc1w, (size_t)k.rd * H); A(k.fc1b, k.rd); A(k.fc2w, H * k.rd); A(k.fc2b, H);
                A(k.w3, H * H); A(k.n3w, H); A(k.n3b, H);
                if (k.cin != (int)H) { A(k.wd, H * k.cin); A(k.ndw, H); A(k.ndb, H); } else { k.wd = k.ndw = k.ndb = nullptr; }
            }
        A(c->stc_w3d, 8 * H * H); A(c->stc_b3d, H); A(c->stc_r0w, H * H); A(c->stc_r0b, H); A(c->stc_r2w, H * H); A(c->stc_r2b, H);
        const size_t rows = (size_t)cfg->max_frames * c->GG;
        const int g2 = c->G / 2 + 1;
        const size_t rows2 = (size_t)(cfg->max_frames / 2 + 1) * g2 * g2;
        A(c->stc_x, rows * H); A(c->stc_y, rows * H); A(c->stc_z, rows * H); A(c->stc_sc, rows * H);
        A(c->stc_col, rows2 * 8 * H); A(c->stc_pool, 32 * H); A(c->stc_g1, 32 * H); A(c->stc_g2, 32 * H); A(c->stc_tmp, 8 * H * H);
    }
    A(c->embed, (size_t)c->V * H); A(c->final_norm, H); A(c->wheads, (size_t)c->NVpad * H);
    A(c->time_tab, (size_t)c->Tv * H); A(c->score_tab, (size_t)c->Sv * H); A(c->sync_row, H);
    c->llm.resize(c->NL);
    const size_t w4_elems[4] = {(size_t)c->QKV * H, H * H, 2 * I * H, H * I};     // qkv, o, gate|up, down
    for (auto& l : c->llm) {
        if (c->w4) {         // 4 bits a weight + a byte per 32: the only copy of the four projections
            A(l.rms1, H); A(l.rms2, H);
            for (int p = 0; p < 4; ++p) { A(l.w4c[p], w4_elems[p] / 2); A(l.w4e[p], w4_elems[p] / 32); }
            continue;
        }
        A(l.rms1, H); A(l.wqkv, (size_t)c->QKV * H); A(l.wo, H * H); A(l.rms2, H); A(l.wgu, 2 * I * H); A(l.wd, H * I);
        A(l.wqkv_d, (size_t)c->QKV * H); A(l.wo_d, H * H); A(l.wgu_d, 2 * I * H); A(l.wd_d, H * I);
        if (c->fp8) {
            A(l.wqkv8, (size_t)c->QKV * H); A(l.wo8, H * H); A(l.wgu8, 2 * I * H); A(l.wd8, H * I);
            A(l.wqkv8_d, (size_t)c->QKV * H); A(l.wo8_d, H * H); A(l.wgu8_d, 2 * I * H); A(l.wd8_d, H * I);
            A(l.sqkv, (size_t)c->QKV); A(l.so, H); A(l.sgu, 2 * I); A(l.sd, H);
        }
    }
    if (c->w4) {
        for (int p = 0; p < 4; ++p) A(c->w4_row[p], w4_elems[p]);
        const size_t piece = std::max(std::max((size_t)c->QKV * H, H * H), H * I);        // the largest tensor a load call brings (gate and up come apart)
        A(c->w4_stage_c, piece / 2); A(c->w4_stage_e, piece / 32);
    }
    A(c->slot_cos, (size_t)c->GG * vh / 2); A(c->slot_sin, (size_t)c->GG * vh / 2);
    A(c->rope_cos, (size_t)c->max_ctx * c->HD / 2); A(c->rope_sin, (size_t)c->max_ctx * c->HD / 2);
    // --- KV cache ---
    c->kv_head_stride = (size_t)c->ctx_pad * c->HD;
    c->slot_stride = c->kv_head_stride * c->NKV;
    c->layer_stride = c->slot_stride * c->max_B;
    if (c->kv8) {
        A(c->k8cache, c->layer_stride * c->NL); A(c->v8cache, c->layer_stride * c->NL);
        A(c->kscache, c->layer_stride / c->HD * c->NL); A(c->vscache, c->layer_stride / c->HD * c->NL);
        A(c->kv_stage_k, c->slot_stride * PF_MAX_N); A(c->kv_stage_v, c->slot_stride * PF_MAX_N);
        A(c->d_ident, MAX_SLOTS);
        c->kcache = c->vcache = nullptr;
    } else { A(c->kcache, c->layer_stride * c->NL); A(c->vcache, c->layer_stride * c->NL); }
    // --- ViT workspaces ---
    const size_t Tm = cfg->max_frames, Tv_ = c->vit_frames, Mv = Tv_ * c->NT;      // tower workspaces: vit_batch_frames at a time
    A(c->vX, Mv * vh); A(c->vH, Mv * vh); A(c->vQKV, Mv * 3 * vh); A(c->vVT, Tv_ * vh * c->tokpad);
    {
        const size_t mlp = Mv * vi, im2 = Tv_ * c->GG * c->Kpad;
        A(c->vMLP, mlp > im2 ? mlp : im2);
    }
    A(c->sl_res, Tm * c->S * vh); A(c->sl_out, Tm * c->S * H);
    if (!c->stc) { c->sl_ws_floats = launch_slot_pool_ws_floats((int)Tm, (int)vh); A(c->sl_ws, c->sl_ws_floats); }
    {
        const int g2 = c->G / 2 + 1;
        const size_t vr = c->stc ? (size_t)(Tm / 2 + 1) * g2 * g2 : Tm * c->TPF;
        A(c->video, vr * H);
    }
    // --- prefill workspaces ---
    const size_t Lm = c->max_ctx;
    // prefill workspaces hold PF_MAX sequences (trace_llm_prefill_pair / _multi)
    const size_t PR = pf_rows(c->max_ctx);
    A(c->pX, PR * H); A(c->pH, PR * H); A(c->pQKV, PR * c->QKV);
    A(c->pO, PR * H); A(c->pACT, PR * I);
    A(c->d_kind, Lm); A(c->d_row, Lm);
    if (c->fp8) { A(c->pA8, PR * std::max(H, I)); A(c->psa, PR); A(c->dA8, (size_t)SK_ROWS * std::max(H, I)); A(c->dsa, SK_ROWS); A(c->dH8, (size_t)SK_ROWS * H); A(c->dsh, SK_ROWS); }
    // --- decode ---
    A(c->dX, SK_ROWS * H); A(c->dH, SK_ROWS * H); A(c->dQKV, SK_ROWS * (size_t)c->QKV); A(c->dO, SK_ROWS * H); A(c->dACT, SK_ROWS * I);
    A(c->xlast, (size_t)std::max(c->max_B, 64) * H);
    A(c->attn_ws, (size_t)SK_ROWS * c->NQ * c->nsplit * (c->HD + 2)); A(c->tickets, SK_ROWS * c->NKV);
    {
        // the partial rows of the four projections, for every kind of GEMV this context can run and (qkv, o, down) for the split-K GEMM of batches above
        // SKINNY_ROWS; beside them what the ticket merge of the bf16 qkv (EPI_NONE) and gate|up (EPI_SWIGLU) GEMVs parks
        const struct { int N, K; bool wide_partial; } proj[4] = {{c->QKV, (int)H, true}, {(int)H, (int)H, true}, {2 * (int)I, (int)H, false}, {(int)H, (int)I, true}};
        size_t f = std::max(skinny_ws_floats(c->QKV, (int)H, EPI_NONE), skinny_ws_floats(2 * (int)I, (int)H, EPI_SWIGLU));
        for (const auto& p : proj) {
            for (SkinnyKind kind : {SK_BF16, SK_W8A8, SK_W8A16})
                if (kind == SK_BF16 || c->fp8) f = std::max(f, skinny_partial_floats(kind, p.N, p.K));
            if (c->w4) f = std::max(f, skinny_partial_floats(SK_W4A16, p.N, p.K));
            if (p.wide_partial) f = std::max(f, (size_t)gemm_partial_ks(p.N, p.K) * SK_ROWS * p.N);
        }
        c->sk_ws_floats = std::max<size_t>(f, 64);
        c->sk_ntickets = (int)std::max<size_t>(std::max<size_t>((size_t)c->QKV, (size_t)H), (size_t)(2 * I)) / 16;
        A(c->sk_ws, c->sk_ws_floats); A(c->sk_tickets, c->sk_ntickets);
        A(c->sk_ws2, c->sk_ws_floats); A(c->dX2, SK_ROWS * H);
    }
    c->ntiles = c->NVpad / 16;
    A(c->part_val, (size_t)SK_ROWS * c->ntiles); A(c->part_idx, (size_t)SK_ROWS * c->ntiles);
    // trace_llm_head_logits: its own arg-max partials and three constant head-id rows (all 0 / all 1 / all 2), so that it shares nothing with a
    // decode batch in flight on another stream and needs no host copy or synchronisation per call
    A(c->hl_val, (size_t)SK_ROWS * c->ntiles); A(c->hl_idx, (size_t)SK_ROWS * c->ntiles);
    A(c->d_heads_tmp, 3 * SK_ROWS); A(c->d_slots, SK_ROWS); A(c->d_pos, SK_ROWS); A(c->d_heads, SK_ROWS); A(c->d_done, SK_ROWS); A(c->d_out_len, SK_ROWS); A(c->d_row_id, SK_ROWS); A(c->d_step0, SK_ROWS); A(c->d_step, 4); A(c->d_params, 4); A(c->d_sparams, 1); A(c->d_lgparams, 1);
    A(c->d_row_sp, SK_ROWS); A(c->d_row_lp, SK_ROWS); A(c->d_row_max, SK_ROWS);
    A(c->d_out_ids, (size_t)SK_ROWS * cfg->max_new_tokens); A(c->d_forced, (size_t)SK_ROWS * cfg->max_new_tokens);
#undef A
    if (rc == TRACE_OK && hipHostMalloc((void**)&c->h_ring, Lm * 8 * trace_ctx::NSTAGE_H) != hipSuccess) rc = fail(TRACE_ERR_HIP, "hipHostMalloc");
    if (rc != TRACE_OK) { trace_ctx_destroy(c); return rc; }
    if (c->kv8) {
        std::vector<int32_t> ident(MAX_SLOTS);
        for (int i = 0; i < MAX_SLOTS; ++i) ident[i] = i;
        if (hipMemcpy(c->d_ident, ident.data(), MAX_SLOTS * 4, hipMemcpyHostToDevice) != hipSuccess) { trace_ctx_destroy(c); return fail(TRACE_ERR_HIP, "hipMemcpy"); }
    }
    c->h_len = Lm;
    c->h_kind = c->h_ring; c->h_row = c->h_kind + Lm;
    for (int i = 0; i < trace_ctx::NSTAGE_H; ++i) hipEventCreateWithFlags(&c->h_ev[i], hipEventDisableTiming);
    hipStreamCreateWithFlags(&c->cap_stream, hipStreamNonBlocking);
    hipEventCreate(&c->ev0); hipEventCreate(&c->ev1);
    hipEventCreate(&c->mev0); hipEventCreate(&c->mev1);
    for (auto& e : c->vev) hipEventCreate(&e);
    c->kev.resize(1024);
    for (auto& e : c->kev) hipEventCreate(&e);
    if (device_id >= 0 && device_id < 16) { g_ctx_per_dev[device_id] += 1; c->counted = true; }
    *out = c;
    return TRACE_OK;
}

extern "C" int trace_ctx_destroy(trace_ctx* c) {
    if (!c) return TRACE_OK;
    (void)hipSetDevice(c->dev);       // the calling thread's current device may be another GPU: everything below (and the counters' key) is this context's
    hipDeviceSynchronize();
    for (auto& st : c->streams) { gemm_pers_forget(st); hipStreamDestroy(st); }
    for (auto& row : c->graphs) for (auto& e : row) for (auto& g : e) if (g.exec) hipGraphExecDestroy(g.exec);
    for (auto& e : c->kev) if (e) hipEventDestroy(e);
    for (auto& e : c->vev) if (e) hipEventDestroy(e);
    if (c->mev0) hipEventDestroy(c->mev0);
    if (c->mev1) hipEventDestroy(c->mev1);
    for (void* p : c->allocs) hipFree(p);
    if (c->pp_buf) hipFree(c->pp_buf);
    if (c->h_ring) hipHostFree(c->h_ring);
    for (int i = 0; i < trace_ctx::NSTAGE_H; ++i) if (c->h_ev[i]) hipEventDestroy(c->h_ev[i]);
    if (c->cap_stream) hipStreamDestroy(c->cap_stream);
    if (c->ev0) hipEventDestroy(c->ev0);
    if (c->ev1) hipEventDestroy(c->ev1);
    if (c->counted && c->dev >= 0 && c->dev < 16 && --g_ctx_per_dev[c->dev] == 0) gemm_pers_release(c->dev);
    delete c;
    return TRACE_OK;
}

extern "C" int64_t trace_ctx_device_bytes(trace_ctx* c) { return c ? (int64_t)c->total_bytes : 0; }

// ------------------------------------------------------------------------------------------------ weights
static int copy2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, int on_device) {
    HIPCHK(hipMemcpy2D(dst, dpitch, src, spitch, width, height, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    return TRACE_OK;
}
static int copy1d(void* dst, const void* src, size_t bytes, int on_device) {
    HIPCHK(hipMemcpy(dst, src, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    return TRACE_OK;
}
static bool starts(const std::string& s, const char* p) { return s.compare(0, strlen(p), p) == 0; }

extern "C" int trace_ctx_load_tensor(trace_ctx* c, const char* name_, const void* data, int on_device, const int64_t* shape,
                                     int ndim) {
    if (!c || !name_ || !data) return fail(TRACE_ERR_ARG, "null argument");
    std::string name(name_);
    int64_t numel = 1;
    for (int i = 0; i < ndim; ++i) numel *= shape[i];
    const size_t H = c->H, I = c->I, vh = c->vh, vi = c->vi, E = sizeof(bf16_t);
    auto expect = [&](int64_t n) -> int {
        if (numel != n) return fail(TRACE_ERR_ARG, "tensor " + name + ": expected " + std::to_string(n) + " elements, got " + std::to_string(numel));
        return TRACE_OK;
    };
    auto done = [&]() { c->loaded[name] = 1; return TRACE_OK; };
    auto flat = [&](bf16_t* dst, int64_t n) -> int { TRY(expect(n)); TRY(copy1d(dst, data, n * E, on_device)); return done(); };

    if (name == "model.embed_tokens.weight") return flat(c->embed, (int64_t)c->V * H);
    if (name == "model.norm.weight") return flat(c->final_norm, H);
    if (name == "lm_head.weight") return flat(c->wheads, (int64_t)c->V * H);
    if (name == "sync_head.weight") return flat(c->wheads + (size_t)c->V * H, H);
    if (name == "time_head.weight") return flat(c->wheads + (size_t)(c->V + 1) * H, (int64_t)c->Tv * H);
    if (name == "score_head.weight") return flat(c->wheads + (size_t)(c->V + 1 + c->Tv) * H, (int64_t)c->Sv * H);
    if (name == "model.time_tower.embed_tokens.weight") return flat(c->time_tab, (int64_t)c->Tv * H);
    if (name == "model.score_tower.embed_tokens.weight") return flat(c->score_tab, (int64_t)c->Sv * H);
    if (name == "model.sync_tower.embed_tokens.weight") return flat(c->sync_row, H);
    if (c->stc && starts(name, "model.mm_projector.")) {
        const std::string k = name.substr(strlen("model.mm_projector."));
        if (k == "sampler.0.bias") return flat(c->stc_b3d, H);
        if (k == "readout.0.weight") return flat(c->stc_r0w, H * H);
        if (k == "readout.0.bias") return flat(c->stc_r0b, H);
        if (k == "readout.2.weight") return flat(c->stc_r2w, H * H);
        if (k == "readout.2.bias") return flat(c->stc_r2b, H);
        if (k == "sampler.0.weight") {      // [Co, Ci, 2,2,2] -> [Co][tap][Ci] for the im2col GEMM
            TRY(expect(8 * (int64_t)H * H));
            TRY(copy1d(c->stc_tmp, data, 8 * H * H * E, on_device));
            if (launch_permute_conv3d_w(c->stc_tmp, c->stc_w3d, (int)H, (int)H, 0) != TRACE_OK) return fail(TRACE_ERR_HIP, "permute launch");
            HIPCHK(hipDeviceSynchronize());
            return done();
        }
        if (k.size() > 6 && (k[0] == 's') && (k[1] == '1' || k[1] == '2') && k[2] == '.' && k[3] == 'b' && k[5] == '.') {
            const int st = k[1] - '1', b = k[4] - '1';
            if (b < 0 || b > 3) return fail(TRACE_ERR_ARG, "bad STC block in " + name);
            StcBlock& q = c->stc_blk[st][b];
            const std::string t = k.substr(6);
            if (t == "conv1.conv.weight") return flat(q.w1, (int64_t)H * q.cin);
            if (t == "conv1.bn.weight") return flat(q.n1w, H);
            if (t == "conv1.bn.bias") return flat(q.n1b, H);
            if (t == "conv2.conv.weight") return flat(q.wdw, H * 9);
            if (t == "conv2.bn.weight") return flat(q.n2w, H);
            if (t == "conv2.bn.bias") return flat(q.n2b, H);
            if (t == "se.fc1.weight") return flat(q.fc1w, (int64_t)q.rd * H);
            if (t == "se.fc1.bias") return flat(q.fc1b, q.rd);
            if (t == "se.fc2.weight") return flat(q.fc2w, (int64_t)H * q.rd);
            if (t == "se.fc2.bias") return flat(q.fc2b, H);
            if (t == "conv3.conv.weight") return flat(q.w3, H * H);
            if (t == "conv3.bn.weight") return flat(q.n3w, H);
            if (t == "conv3.bn.bias") return flat(q.n3b, H);
            if (q.wd && t == "downsample.conv.weight") return flat(q.wd, (int64_t)H * q.cin);
            if (q.wd && t == "downsample.bn.weight") return flat(q.ndw, H);
            if (q.wd && t == "downsample.bn.bias") return flat(q.ndb, H);
        }
        return fail(TRACE_ERR_ARG, "unknown tensor " + name);
    }
    if (name == "model.mm_projector.slots") return flat(c->sl_slots, (int64_t)vh * c->S);
    if (name == "model.mm_projector.ln_vision.weight") return flat(c->sl_lnw, vh);
    if (name == "model.mm_projector.ln_vision.bias") return flat(c->sl_lnb, vh);
    if (name == "model.mm_projector.readout.weight") return flat(c->sl_readout, (int64_t)H * vh);

    if (starts(name, "model.layers.")) {
        const char* p = name.c_str() + strlen("model.layers.");
        char* end = nullptr;
        const long l = strtol(p, &end, 10);
        if (l < 0 || l >= c->NL || *end != '.') return fail(TRACE_ERR_ARG, "bad layer index in " + name);
        const std::string k(end + 1);
        LlmLayer& L = c->llm[l];
        const size_t qrows = (size_t)c->NQ * c->HD, kvrows = (size_t)c->NKV * c->HD;
        if (k == "input_layernorm.weight") return flat(L.rms1, H);
        if (k == "post_attention_layernorm.weight") return flat(L.rms2, H);
        if (c->w4) {
            // a projection piece of `rows` rows lands in the layer scratch of its projection, is quantised row-wise into the staging arrays and packed into
            // tiles tile0, tile0 + step, ... of the layer's only copy (gate / up: alternating tiles, the 16-row interleave of the 16-bit path)
            auto piece = [&](int p, size_t rows, size_t K, size_t tile0, int step) -> int {
                TRY(expect((int64_t)(rows * K)));
                TRY(copy1d(c->w4_row[p], data, rows * K * E, on_device));
                LCHK(launch_quant_rows_w4(c->w4_row[p], (long)K, c->w4_stage_c, c->w4_stage_e, (int)rows, (int)K, 0));
                LCHK(launch_tile_pack_w4(c->w4_stage_c, c->w4_stage_e, L.w4c[p], L.w4e[p], (int)rows, (int)K, (int)tile0, step, 0));
                HIPCHK(hipDeviceSynchronize());
                return done();
            };
            if (k == "self_attn.q_proj.weight") return piece(0, qrows, H, 0, 1);
            if (k == "self_attn.k_proj.weight") return piece(0, kvrows, H, qrows / 16, 1);
            if (k == "self_attn.v_proj.weight") return piece(0, kvrows, H, (qrows + kvrows) / 16, 1);
            if (k == "self_attn.o_proj.weight") return piece(1, H, H, 0, 1);
            if (k == "mlp.gate_proj.weight") return piece(2, I, H, 0, 2);
            if (k == "mlp.up_proj.weight") return piece(2, I, H, 1, 2);
            if (k == "mlp.down_proj.weight") return piece(3, H, I, 0, 1);
            return fail(TRACE_ERR_ARG, "unknown tensor " + name);
        }
        if (k == "self_attn.q_proj.weight") return flat(L.wqkv, qrows * H);
        if (k == "self_attn.k_proj.weight") return flat(L.wqkv + qrows * H, kvrows * H);
        if (k == "self_attn.v_proj.weight") return flat(L.wqkv + (qrows + kvrows) * H, kvrows * H);
        if (k == "self_attn.o_proj.weight") return flat(L.wo, H * H);
        if (k == "mlp.down_proj.weight") return flat(L.wd, H * I);
        if (k == "mlp.gate_proj.weight" || k == "mlp.up_proj.weight") {
            // interleave 16-row groups: packed rows [32t, 32t+16) = gate[16t..], [32t+16, 32t+32) = up[16t..]
            TRY(expect(I * H));
            bf16_t* dst = L.wgu + (k == "mlp.up_proj.weight" ? 16 * H : 0);
            TRY(copy2d(dst, 32 * H * E, data, 16 * H * E, 16 * H * E, I / 16, on_device));
            return done();
        }
        return fail(TRACE_ERR_ARG, "unknown tensor " + name);
    }

    // vision tower: accept both transformers key layouts (with / without ".vision_model")
    const char* vp1 = "model.vision_tower.vision_tower.vision_model.";
    const char* vp2 = "model.vision_tower.vision_tower.";
    std::string k;
    if (starts(name, vp1)) k = name.substr(strlen(vp1));
    else if (starts(name, vp2)) k = name.substr(strlen(vp2));
    else return fail(TRACE_ERR_ARG, "unknown tensor " + name);
    auto vdone = [&](const std::string& canon) { c->loaded[std::string(vp1) + canon] = 1; return TRACE_OK; };
    auto vflat = [&](bf16_t* dst, int64_t n) -> int { TRY(expect(n)); TRY(copy1d(dst, data, n * E, on_device)); return vdone(k); };
    if (k == "embeddings.class_embedding") return vflat(c->cls, vh);
    if (k == "embeddings.position_embedding.weight") return vflat(c->pos_emb, (int64_t)c->NT * vh);
    if (k == "embeddings.patch_embedding.weight") {
        TRY(expect((int64_t)vh * c->Kpatch));
        TRY(copy2d(c->patch_w, c->Kpad * E, data, c->Kpatch * E, c->Kpatch * E, vh, on_device));
        return vdone(k);
    }
    if (k == "pre_layrnorm.weight") return vflat(c->pre_w, vh);
    if (k == "pre_layrnorm.bias") return vflat(c->pre_b, vh);
    if (starts(k, "post_layernorm.") || k == "embeddings.position_ids") return 1;       // unused on this path
    if (starts(k, "encoder.layers.")) {
        const char* p = k.c_str() + strlen("encoder.layers.");
        char* end = nullptr;
        const long l = strtol(p, &end, 10);
        if (l < 0 || *end != '.') return fail(TRACE_ERR_ARG, "bad layer index in " + name);
        if (l >= c->vL) return 1;     // layers after the selected hidden state never run (select_layer = -2)
        const std::string kk(end + 1);
        VitLayer& L = c->vit[l];
        if (kk == "layer_norm1.weight") return vflat(L.ln1w, vh);
        if (kk == "layer_norm1.bias") return vflat(L.ln1b, vh);
        if (kk == "layer_norm2.weight") return vflat(L.ln2w, vh);
        if (kk == "layer_norm2.bias") return vflat(L.ln2b, vh);
        if (kk == "self_attn.q_proj.weight") return vflat(L.wqkv, vh * vh);
        if (kk == "self_attn.k_proj.weight") return vflat(L.wqkv + vh * vh, vh * vh);
        if (kk == "self_attn.v_proj.weight") return vflat(L.wqkv + 2 * vh * vh, vh * vh);
        if (kk == "self_attn.q_proj.bias") return vflat(L.bqkv, vh);
        if (kk == "self_attn.k_proj.bias") return vflat(L.bqkv + vh, vh);
        if (kk == "self_attn.v_proj.bias") return vflat(L.bqkv + 2 * vh, vh);
        if (kk == "self_attn.out_proj.weight") return vflat(L.wo, vh * vh);
        if (kk == "self_attn.out_proj.bias") return vflat(L.bo, vh);
        if (kk == "mlp.fc1.weight") return vflat(L.w1, vi * vh);
        if (kk == "mlp.fc1.bias") return vflat(L.b1, vi);
        if (kk == "mlp.fc2.weight") return vflat(L.w2, vh * vi);
        if (kk == "mlp.fc2.bias") return vflat(L.b2, vh);
    }
    return fail(TRACE_ERR_ARG, "unknown tensor " + name);
}

extern "C" int trace_ctx_finalize(trace_ctx* c) {
    if (!c) return fail(TRACE_ERR_ARG, "null ctx");
    const int expected = (c->stc ? 9 + 8 * 13 + 3 + 6 : 13) + 9 * c->NL + 5 + 16 * c->vL;
    if ((int)c->loaded.size() != expected)
        return fail(TRACE_ERR_STATE, "weights incomplete: " + std::to_string(c->loaded.size()) + " of " + std::to_string(expected) + " tensors loaded");
    // RoPE tables, computed the way the reference does (fp32 inv_freq, fp32 angle, cos/sin of that angle)
    {
        const int d = c->vh, h2 = d / 2, n = c->GG;
        std::vector<float> cs((size_t)n * h2), sn((size_t)n * h2);
        for (int j = 0; j < h2; ++j) {
            const float inv = 1.0f / (float)pow((double)c->c.slot_rope_base, (double)((float)(2 * j) / (float)d));
            for (int t = 0; t < n; ++t) {
                const float ang = (float)t * inv;
                cs[(size_t)t * h2 + j] = (float)cos((double)ang);
                sn[(size_t)t * h2 + j] = (float)sin((double)ang);
            }
        }
        HIPCHK(hipMemcpy(c->slot_cos, cs.data(), cs.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(c->slot_sin, sn.data(), sn.size() * 4, hipMemcpyHostToDevice));
    }
    {
        const int d = c->HD, h2 = d / 2, n = c->max_ctx;
        std::vector<float> cs((size_t)n * h2), sn((size_t)n * h2);
        for (int j = 0; j < h2; ++j) {
            const float inv = 1.0f / (float)pow((double)c->c.rope_theta, (double)((float)(2 * j) / (float)d));
            for (int t = 0; t < n; ++t) {
                const float ang = (float)t * inv;
                cs[(size_t)t * h2 + j] = (float)cos((double)ang);
                sn[(size_t)t * h2 + j] = (float)sin((double)ang);
            }
        }
        HIPCHK(hipMemcpy(c->rope_cos, cs.data(), cs.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(c->rope_sin, sn.data(), sn.size() * 4, hipMemcpyHostToDevice));
    }
    // fused patch embedding: the conv weight in the kernel's k order / fragment layout, and the CLS row (the same for every frame)
    if (c->patch_wp) {
        LCHK(launch_patch_pack(c->patch_w, c->Kpad, c->patch_wp, c->vh, c->P, 0));
        LCHK(launch_cls_row(c->cls, c->pos_emb, c->pre_w, c->pre_b, c->cls_row, c->vh, c->c.v_eps, 0));
    }
    // decode copies of the LLM matrices in the GEMV tile layout (288 GB of HBM: +14.5 GB buys ~25% on the weight stream)
    for (auto& l : c->llm) {
        if (c->w4) break;                                 // packed as the tensors arrived
        LCHK(launch_tile_pack(l.wqkv, c->H, l.wqkv_d, c->QKV, c->H, 0));
        LCHK(launch_tile_pack(l.wo, c->H, l.wo_d, c->H, c->H, 0));
        LCHK(launch_tile_pack(l.wgu, c->H, l.wgu_d, 2 * c->I, c->H, 0));
        LCHK(launch_tile_pack(l.wd, c->I, l.wd_d, c->H, c->I, 0));
        if (c->fp8) {      // per-output-row e4m3 quantisation of the four projections (from the bf16 copies), then the decode tile layout
            LCHK(launch_quant_rows_fp8(l.wqkv, c->H, l.wqkv8, c->H, l.sqkv, c->QKV, c->H, 0));
            LCHK(launch_quant_rows_fp8(l.wo, c->H, l.wo8, c->H, l.so, c->H, c->H, 0));
            LCHK(launch_quant_rows_fp8(l.wgu, c->H, l.wgu8, c->H, l.sgu, 2 * c->I, c->H, 0));
            LCHK(launch_quant_rows_fp8(l.wd, c->I, l.wd8, c->I, l.sd, c->H, c->I, 0));
            LCHK(launch_tile_pack_fp8(l.wqkv8, c->H, l.wqkv8_d, c->QKV, c->H, 0));
            LCHK(launch_tile_pack_fp8(l.wo8, c->H, l.wo8_d, c->H, c->H, 0));
            LCHK(launch_tile_pack_fp8(l.wgu8, c->H, l.wgu8_d, 2 * c->I, c->H, 0));
            LCHK(launch_tile_pack_fp8(l.wd8, c->I, l.wd8_d, c->H, c->I, 0));
        }
    }
    {
        int32_t h[3 * SK_ROWS];
        for (int i = 0; i < 3 * SK_ROWS; ++i) h[i] = i / SK_ROWS;
        HIPCHK(hipMemcpy(c->d_heads_tmp, h, sizeof(h), hipMemcpyHostToDevice));
    }
    // ticket counters of the persistent GEMM for the streams this context launches on by itself (an allocation + a memset: not something to
    // meet inside a timed or captured region); a caller's own stream gets its counters at its first launch
    HIPCHK(hipSetDevice(c->dev));
    if (gemm_pers_init(nullptr) != TRACE_OK || gemm_pers_init(c->cap_stream) != TRACE_OK) return fail(TRACE_ERR_HIP, "persistent GEMM ticket counters");
    HIPCHK(hipDeviceSynchronize());
    c->finalized = true;
    return TRACE_OK;
}

// ------------------------------------------------------------------------------------------------ ViT
static unsigned long long* g_gemm_trace = nullptr;      // tools/gemm_trace.py
extern "C" int trace_op_set_gemm_trace(void* buf) { g_gemm_trace = (unsigned long long*)buf; return TRACE_OK; }
static int gemm_checked(const GemmArgs& g, int epi, hipStream_t s, const char* what) {       // launch_gemm_bf16, a failure recorded with its shape
    const int rc = launch_gemm_bf16(g, epi, s);
    if (rc != TRACE_OK) return fail(rc, std::string(what) + " launch failed (M=" + std::to_string(g.M) + " N=" + std::to_string(g.N) + " K=" + std::to_string(g.K) + ")");
    return TRACE_OK;
}
static int gemm(const bf16_t* A, int lda, const bf16_t* W, int ldw, bf16_t* C, int ldc, const bf16_t* bias, const bf16_t* R,
                int ldr, int M, int N, int K, int epi, hipStream_t s) {
    GemmArgs g{A, lda, W, ldw, C, ldc, bias, R, ldr, M, N, K, g_gemm_trace, 0, nullptr, nullptr};
    return gemm_checked(g, epi, s, "gemm");
}

// C = (quantise_rows(A) . W8^T) * scales (+ epilogue): A [M,K] bf16 is quantised row-wise into c->pA8 / c->psa first
static int gemm_fp8(trace_ctx* c, const bf16_t* A, int lda, const uint8_t* W8, const float* sw, bf16_t* C, int ldc, const bf16_t* R, int ldr,
                    int M, int N, int K, int epi, hipStream_t s) {
    LCHK(launch_quant_rows_fp8(A, lda, c->pA8, K, c->psa, M, K, s));
    GemmArgs g{reinterpret_cast<const bf16_t*>(c->pA8), K, reinterpret_cast<const bf16_t*>(W8), K, C, ldc, nullptr, R, ldr, M, N, K, nullptr, 1, c->psa, sw};
    return gemm_checked(g, epi, s, "fp8 gemm");
}

extern "C" int trace_vit_forward(trace_ctx* c, const void* frames, int frames_dtype, int T, void* feats_out, void* stream) {
    if (!c || !c->finalized) return fail(TRACE_ERR_STATE, "context not finalized");
    if (!frames || T < 1 || T > c->vit_frames) return fail(TRACE_ERR_ARG, "bad frames / T (more than max_frames / vit_batch_frames)");
    hipStream_t s = (hipStream_t)stream;
    const int vh = c->vh, vi = c->vi, NT = c->NT, GG = c->GG, Mv = T * NT;
    // front end: one kernel reads the frame tensor, multiplies the patches on the MFMA, adds CLS / position embeddings and applies
    // pre_layrnorm (patch_embed.hip).  vit.patch_fused = 0 (A/B) or a patch size / width the kernel does not take: the round-1 path,
    // im2col matrix -> GEMM -> assemble.
    const bool fused_pe = g_tune.vit_patch_fused && c->patch_wp;
    if (fused_pe) {
        LCHK(launch_patch_embed(frames, frames_dtype == 1, c->patch_wp, c->pos_emb, c->pre_w, c->pre_b, c->cls_row, c->vX, T, c->c.v_image, c->P, vh,
                                c->c.v_eps, s));
    } else {
        bf16_t* im2 = c->vMLP;                       // [T*GG, Kpad]
        bf16_t* pe = c->vH;                          // [T*GG, vh]
        LCHK(launch_im2col(frames, frames_dtype == 1, im2, T, c->c.v_image, c->P, c->Kpad, s));
        TRY(gemm(im2, c->Kpad, c->patch_w, c->Kpad, pe, vh, nullptr, nullptr, 0, T * GG, vh, c->Kpad, EPI_NONE, s));
        LCHK(launch_vit_assemble(pe, c->cls, c->pos_emb, c->pre_w, c->pre_b, c->vX, T, GG, vh, c->c.v_eps, s));
    }
    AttnArgs a{};
    a.Q = c->vQKV; a.K = c->vQKV + vh; a.V = c->vVT; a.O = c->vH;
    a.q_bs = (long)NT * 3 * vh; a.q_hs = 64; a.q_rs = 3 * vh;
    a.k_bs = a.q_bs; a.k_hs = 64; a.k_rs = 3 * vh;
    a.v_bs = (long)vh * c->tokpad; a.v_hs = 64L * c->tokpad; a.v_rs = c->tokpad;
    a.o_bs = (long)NT * vh; a.o_hs = 64; a.o_rs = vh;
    a.nq_rows = NT; a.nkv_rows = NT; a.batch = T; a.heads = c->vheads; a.kv_heads = c->vheads;
    a.scale = 0.125f; a.causal = 0;
    a.Vrow = c->vQKV + 2 * vh; a.vr_bs = a.q_bs; a.vr_hs = 64; a.vr_rs = 3 * vh;
    a.v_perm = attn_vit_wants_perm(NT, true) ? (attn_vit_rowmajor_v() ? 2 : 1) : 0;     // 2: V read row-major from vQKV, no transpose pass
    for (int l = 0; l < c->vL; ++l) {
        const VitLayer& L = c->vit[l];
        // MFMA roofline probe (profile == 2): HIP events around ONE launch of each of the layer's four GEMM shapes, in layer 0, per call — of the
        // largest call shape seen since trace_set_profile only (the short tail call of a frame stream would mix two shapes into one average).
        // The fc1 pair (mev0 / mev1) is the `roofline` object's bracket; pairs 0..2 of vev are qkv, out-proj and fc2.
        const bool vprof = c->profile == 2 && (c->bracket_mask & 1);
        if (l == 0 && vprof && Mv > c->mM) { c->mM = Mv; c->msum_ms = 0.0; c->msamples = 0; c->vsum_ms[0] = c->vsum_ms[1] = c->vsum_ms[2] = 0.0; }
        const bool probe = (l == 0 && vprof && Mv == c->mM);
#define VPROBE_BEGIN(i) if (probe) hipEventRecord(c->vev[2 * (i)], s)
#define VPROBE_END(i, N_, K_) if (probe) { hipEventRecord(c->vev[2 * (i) + 1], s); c->vflops[i] = 2.0 * Mv * (double)(N_) * (K_); }
        LCHK(launch_layernorm(c->vX, vh, c->vH, vh, L.ln1w, L.ln1b, Mv, vh, c->c.v_eps, s));
        VPROBE_BEGIN(0);
        TRY(gemm(c->vH, vh, L.wqkv, vh, c->vQKV, 3 * vh, L.bqkv, nullptr, 0, Mv, 3 * vh, vh, EPI_NONE, s));
        VPROBE_END(0, 3 * vh, vh);
        if (a.v_perm != 2)
            LCHK(launch_transpose_v(c->vQKV + 2 * vh, (long)NT * 3 * vh, 64, 3 * vh, c->vVT, a.v_bs, a.v_hs, c->tokpad, NT, 64,
                                    c->vheads, T, s, a.v_perm));
        LCHK(launch_attn_vit(a, s));
        VPROBE_BEGIN(1);
        TRY(gemm(c->vH, vh, L.wo, vh, c->vX, vh, L.bo, c->vX, vh, Mv, vh, vh, EPI_RESIDUAL, s));
        VPROBE_END(1, vh, vh);
        LCHK(launch_layernorm(c->vX, vh, c->vH, vh, L.ln2w, L.ln2b, Mv, vh, c->c.v_eps, s));
        if (probe) hipEventRecord(c->mev0, s);
        TRY(gemm(c->vH, vh, L.w1, vh, c->vMLP, vi, L.b1, nullptr, 0, Mv, vi, vh, EPI_QUICKGELU, s));
        if (probe) { hipEventRecord(c->mev1, s); c->mflops = 2.0 * Mv * (double)vi * vh; }
        VPROBE_BEGIN(2);
        TRY(gemm(c->vMLP, vi, L.w2, vi, c->vX, vh, L.b2, c->vX, vh, Mv, vh, vi, EPI_RESIDUAL, s));
        VPROBE_END(2, vh, vi);
#undef VPROBE_BEGIN
#undef VPROBE_END
    }
    if (c->profile == 2 && (c->bracket_mask & 1) && c->vL > 0 && Mv == c->mM) {
        hipEventSynchronize(c->vev[5]);                       // layer 0's fc2: the last of the bracketed launches
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->mev0, c->mev1) == hipSuccess) { c->msum_ms += ms; c->msamples += 1; }
        for (int i = 0; i < 3; ++i)
            if (hipEventElapsedTime(&ms, c->vev[2 * i], c->vev[2 * i + 1]) == hipSuccess) c->vsum_ms[i] += ms;
        c->prof[5] = (float)(c->msum_ms / c->msamples);
        c->prof[6] = (float)c->msamples;
        c->prof[7] = (float)(c->mflops / 1e9);               // GFLOP of the bracketed launch
        c->prof[9] = 0.f;                                     // (was: LayerNorm fold on / off — the fold left the product in round 5)
        for (int i = 0; i < 3; ++i) { c->prof[12 + i] = (float)(c->vsum_ms[i] / c->msamples); c->prof[15 + i] = (float)(c->vflops[i] / 1e9); }
    }
    if (feats_out)   // drop CLS: [T, GG, vh]
        HIPCHK(hipMemcpy2DAsync(feats_out, (size_t)GG * vh * 2, c->vX + vh, (size_t)NT * vh * 2, (size_t)GG * vh * 2, T,
                                hipMemcpyDeviceToDevice, s));
    return TRACE_OK;
}

extern "C" int trace_slot_pool(trace_ctx* c, const void* feats, int T, void* slots_out, void* stream) {
    if (!c || !c->finalized) return fail(TRACE_ERR_STATE, "context not finalized");
    if (T < 1 || T > c->c.max_frames) return fail(TRACE_ERR_ARG, "bad T");
    if (c->stc) return fail(TRACE_ERR_STATE, "this context holds the STC connector, not SpatialSlotPool");
    hipStream_t s = (hipStream_t)stream;
    const int vh = c->vh;
    const bf16_t* f = feats ? (const bf16_t*)feats : c->vX + vh;
    const long fs = feats ? (long)c->GG * vh : (long)c->NT * vh;
    LCHK(launch_slot_pool(f, fs, vh, c->sl_lnw, c->sl_lnb, c->sl_slots, c->slot_cos, c->slot_sin, c->sl_res, T, c->GG, vh,
                          c->S, c->c.slot_eps, c->sl_ws, c->sl_ws_floats, s));
    TRY(gemm(c->sl_res, vh, c->sl_readout, vh, c->sl_out, c->H, nullptr, nullptr, 0, T * c->S, c->H, vh, EPI_NONE, s));
    if (slots_out) HIPCHK(hipMemcpyAsync(slots_out, c->sl_out, (size_t)T * c->S * c->H * 2, hipMemcpyDeviceToDevice, s));
    return TRACE_OK;
}

// one timm-style RegNet bottleneck on channels-last rows: x [N*HW, cin] -> out [N*HW, H] (out may alias nothing of x)
static int stc_block(trace_ctx* c, const StcBlock& k, const bf16_t* x, bf16_t* out, int N, int hh, int ww, hipStream_t s) {
    const int H = c->H, HW = hh * ww, rows = N * HW;
    bf16_t *y = c->stc_y, *z = c->stc_z, *sc = c->stc_sc;
    TRY(gemm(x, k.cin, k.w1, k.cin, y, H, nullptr, nullptr, 0, rows, H, k.cin, EPI_NONE, s));
    LCHK(launch_layernorm(y, H, y, H, k.n1w, k.n1b, rows, H, 1e-6f, s, 1));
    LCHK(launch_dwconv3x3(y, k.wdw, z, N, hh, ww, H, s));
    LCHK(launch_layernorm(z, H, z, H, k.n2w, k.n2b, rows, H, 1e-6f, s, 1));
    LCHK(launch_avgpool(z, c->stc_pool, N, HW, H, s));
    LCHK(launch_skinny_gemm(c->stc_pool, H, k.fc1w, H, c->stc_g1, k.rd, nullptr, 0, N, k.rd, H, EPI_NONE, 0, SKWS(c), s));
    LCHK(launch_bias_act(c->stc_g1, k.fc1b, N, k.rd, ACT_SILU, s));
    LCHK(launch_skinny_gemm(c->stc_g1, k.rd, k.fc2w, k.rd, c->stc_g2, H, nullptr, 0, N, H, k.rd, EPI_NONE, 0, SKWS(c), s));
    LCHK(launch_bias_act(c->stc_g2, k.fc2b, N, H, ACT_SIGMOID, s));
    LCHK(launch_scale_rows(z, c->stc_g2, N, HW, H, s));
    TRY(gemm(z, H, k.w3, H, y, H, nullptr, nullptr, 0, rows, H, H, EPI_NONE, s));
    const bf16_t* shortcut = x;
    if (k.wd) {
        TRY(gemm(x, k.cin, k.wd, k.cin, sc, H, nullptr, nullptr, 0, rows, H, k.cin, EPI_NONE, s));
        LCHK(launch_layernorm(sc, H, sc, H, k.ndw, k.ndb, rows, H, 1e-6f, s, 0));
        shortcut = sc;
    }
    // out = SiLU(LN(conv3 out) + shortcut) in ONE pass, written where the next block reads it (round 5: was LayerNorm, add + SiLU and a copy —
    // three passes over [rows, H]; same rounding points).  x is dead from here on (out may be x: row-wise in place).
    LCHK(launch_layernorm(y, H, out, H, k.n3w, k.n3b, rows, H, 1e-6f, s, 1, shortcut, H));
    return TRACE_OK;
}

extern "C" int trace_stc_connector(trace_ctx* c, const void* feats, int T, void* out, int* rows_out, void* stream) {
    if (!c || !c->finalized) return fail(TRACE_ERR_STATE, "context not finalized");
    if (!c->stc) return fail(TRACE_ERR_STATE, "context was not created with projector_type = stc_connector");
    if (T < 1 || T > c->c.max_frames || T > 32) return fail(TRACE_ERR_ARG, "bad T");
    hipStream_t s = (hipStream_t)stream;
    const int H = c->H, vh = c->vh, G = c->G, GG = c->GG;
    // gather the patch rows (drop CLS) into a dense [T*GG, vh] buffer
    if (feats) HIPCHK(hipMemcpyAsync(c->stc_x, feats, (size_t)T * GG * vh * 2, hipMemcpyDeviceToDevice, s));
    else HIPCHK(hipMemcpy2DAsync(c->stc_x, (size_t)GG * vh * 2, c->vX + vh, (size_t)c->NT * vh * 2, (size_t)GG * vh * 2, T,
                                 hipMemcpyDeviceToDevice, s));
    // s1: 4 blocks on [T, G, G]; every block reads stc_x and leaves its result there (block 0 reads it with row
    // pitch vh and writes pitch H: the result is produced in stc_y and copied once x is dead)
    for (int b = 0; b < 4; ++b) TRY(stc_block(c, c->stc_blk[0][b], c->stc_x, c->stc_x, T, G, G, s));
    // sampler: Conv3d k = s = 2, p = 1 (+bias) + SiLU as an im2col GEMM
    const int To = T / 2 + 1, Go = G / 2 + 1, rows2 = To * Go * Go;
    LCHK(launch_im2col3d(c->stc_x, c->stc_col, T, G, G, H, To, Go, Go, s));
    TRY(gemm(c->stc_col, 8 * H, c->stc_w3d, 8 * H, c->stc_x, H, c->stc_b3d, nullptr, 0, rows2, H, 8 * H, EPI_NONE, s));
    LCHK(launch_bias_act(c->stc_x, nullptr, rows2, H, ACT_SILU, s));
    for (int b = 0; b < 4; ++b) TRY(stc_block(c, c->stc_blk[1][b], c->stc_x, c->stc_x, To, Go, Go, s));
    // readout MLP
    TRY(gemm(c->stc_x, H, c->stc_r0w, H, c->stc_y, H, c->stc_r0b, nullptr, 0, rows2, H, H, EPI_NONE, s));
    LCHK(launch_bias_act(c->stc_y, nullptr, rows2, H, ACT_GELU, s));
    TRY(gemm(c->stc_y, H, c->stc_r2w, H, c->video, H, c->stc_r2b, nullptr, 0, rows2, H, H, EPI_NONE, s));
    c->video_rows = rows2;
    if (rows_out) *rows_out = rows2;
    if (out) HIPCHK(hipMemcpyAsync(out, c->video, (size_t)rows2 * H * 2, hipMemcpyDeviceToDevice, s));
    return TRACE_OK;
}

// The next pinned staging buffer of the ring (h_kind / h_row point into it afterwards): waits only for the copies that last read THAT buffer, four uses ago —
// normally long done — instead of draining the stream.  stage_release() records the buffer's event behind the copies just queued.
static int stage_acquire(trace_ctx* c) {
    c->h_next = (c->h_next + 1) % trace_ctx::NSTAGE_H;
    HIPCHK(hipEventSynchronize(c->h_ev[c->h_next]));          // (an event never recorded is complete)
    c->h_kind = c->h_ring + (size_t)c->h_next * 2 * c->h_len;
    c->h_row = c->h_kind + c->h_len;
    return TRACE_OK;
}
static int stage_release(trace_ctx* c, hipStream_t s) {
    HIPCHK(hipEventRecord(c->h_ev[c->h_next], s));
    return TRACE_OK;
}

// slot pool on `feats` (nullptr = the tower's internal buffer) + the per-frame time-token rows -> c->video
static int encode_tail(trace_ctx* c, const void* feats, int T, const int32_t* time_ids, void* video_out, void* stream) {
    if (!c || !c->finalized) return fail(TRACE_ERR_STATE, "context not finalized");
    hipStream_t s = (hipStream_t)stream;
    TRY(trace_slot_pool(c, feats, T, nullptr, stream));
    const int rows = T * c->TPF;
    TRY(stage_acquire(c));
    for (int t = 0; t < T; ++t)
        for (int j = 0; j < c->TPF; ++j) {
            const int r = t * c->TPF + j;
            if (j < c->S) { c->h_kind[r] = 0; c->h_row[r] = t * c->S + j; }
            else {
                const int id = time_ids[t * 6 + (j - c->S)];
                if (id < 0 || id >= c->Tv) return fail(TRACE_ERR_ARG, "time id out of range");
                c->h_kind[r] = 1; c->h_row[r] = id;
            }
        }
    HIPCHK(hipMemcpyAsync(c->d_kind, c->h_kind, rows * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->d_row, c->h_row, rows * 4, hipMemcpyHostToDevice, s));
    TRY(stage_release(c, s));
    GatherTabs tabs{};
    tabs.t[0] = c->sl_out; tabs.t[1] = c->time_tab;
    LCHK(launch_gather_rows(tabs, c->d_kind, c->d_row, c->video, rows, c->H, s));
    c->video_rows = rows;
    if (video_out) HIPCHK(hipMemcpyAsync(video_out, c->video, (size_t)rows * c->H * 2, hipMemcpyDeviceToDevice, s));
    return TRACE_OK;
}

extern "C" int trace_encode_video(trace_ctx* c, const void* frames, int frames_dtype, int T, const int32_t* time_ids,
                                  void* video_out, void* stream) {
    if (!time_ids) return fail(TRACE_ERR_ARG, "null time_ids");
    if (c && T > c->c.max_frames) return fail(TRACE_ERR_ARG, "bad T (more frames than max_frames)");
    TRY(trace_vit_forward(c, frames, frames_dtype, T, nullptr, stream));
    return encode_tail(c, nullptr, T, time_ids, video_out, stream);
}

extern "C" int trace_encode_features(trace_ctx* c, const void* feats, int T, const int32_t* time_ids, void* video_out, void* stream) {
    if (!time_ids || !feats) return fail(TRACE_ERR_ARG, "null feats / time_ids");
    return encode_tail(c, feats, T, time_ids, video_out, stream);
}

// the L embedding rows `ids` name (a video placeholder = the rows of the last encode) gathered into pX: the body of trace_splice_embeds / trace_embed_rows
static int splice_rows(trace_ctx* c, const int32_t* ids, int n_ids, const int32_t* time_rows, int n_time, const int32_t* score_rows, int n_score,
                       int L, void* embeds_out, hipStream_t s) {
    TRY(stage_acquire(c));
    int r = 0, ti = 0, si = 0;
    for (int i = 0; i < n_ids; ++i) {
        const int id = ids[i];
        if (id == -201 || id == -200) {
            for (int j = 0; j < c->video_rows; ++j, ++r) { c->h_kind[r] = 1; c->h_row[r] = j; }
        } else if (id == -205) { c->h_kind[r] = 4; c->h_row[r] = 0; ++r; }
        else if (id == -203) {
            if (ti >= n_time || !time_rows) return fail(TRACE_ERR_ARG, "more <time> placeholders than time tokens");
            if (time_rows[ti] < 0 || time_rows[ti] >= c->Tv) return fail(TRACE_ERR_ARG, "time token id out of range");     // nn.Embedding raises
            c->h_kind[r] = 2; c->h_row[r] = time_rows[ti++]; ++r;
        } else if (id == -204) {
            if (si >= n_score || !score_rows) return fail(TRACE_ERR_ARG, "more <score> placeholders than score tokens");
            if (score_rows[si] < 0 || score_rows[si] >= c->Sv) return fail(TRACE_ERR_ARG, "score token id out of range");
            c->h_kind[r] = 3; c->h_row[r] = score_rows[si++]; ++r;
        } else {
            const int t = id < 0 ? 0 : id;      // torch.clamp(ids, min=0) (trace_arch.py:417)
            if (t >= c->V) return fail(TRACE_ERR_ARG, "token id out of range");
            c->h_kind[r] = 0; c->h_row[r] = t; ++r;
        }
    }
    // the masked assignment of trace_arch.py:426-427 fails with a shape mismatch unless every supplied token has its placeholder
    if (ti != n_time || si != n_score) return fail(TRACE_ERR_ARG, "fewer <time>/<score> placeholders than supplied tokens");
    HIPCHK(hipMemcpyAsync(c->d_kind, c->h_kind, L * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->d_row, c->h_row, L * 4, hipMemcpyHostToDevice, s));
    TRY(stage_release(c, s));
    GatherTabs tabs{};
    tabs.t[0] = c->embed; tabs.t[1] = c->video; tabs.t[2] = c->time_tab; tabs.t[3] = c->score_tab; tabs.t[4] = c->sync_row;
    LCHK(launch_gather_rows(tabs, c->d_kind, c->d_row, c->pX, L, c->H, s));
    c->spliced_len = L;
    if (embeds_out) HIPCHK(hipMemcpyAsync(embeds_out, c->pX, (size_t)L * c->H * 2, hipMemcpyDeviceToDevice, s));
    return TRACE_OK;
}

extern "C" int trace_splice_embeds(trace_ctx* c, const int32_t* ids, int n_ids, const int32_t* time_rows, int n_time,
                                   const int32_t* score_rows, int n_score, int* L_out, void* embeds_out, void* stream) {
    if (!c || !c->finalized) return fail(TRACE_ERR_STATE, "context not finalized");
    if (!ids || n_ids < 1) return fail(TRACE_ERR_ARG, "bad ids");
    int nvid = 0;
    for (int i = 0; i < n_ids; ++i) nvid += (ids[i] == -201 || ids[i] == -200);
    if (nvid != 1) return fail(TRACE_ERR_ARG, "only have one video inputs!");          // trace_arch.py:411
    if (c->video_rows <= 0) return fail(TRACE_ERR_STATE, "no encoded video");
    const int L = n_ids - 1 + c->video_rows;
    if (L > c->max_ctx) return fail(TRACE_ERR_ARG, "spliced prompt longer than max_ctx");
    TRY(splice_rows(c, ids, n_ids, time_rows, n_time, score_rows, n_score, L, embeds_out, (hipStream_t)stream));
    if (L_out) *L_out = L;
    return TRACE_OK;
}

// The same gather for rows that hold no video: the part of a prompt after <video>, appended to a cached prefix (trace_llm_prefill_append)
extern "C" int trace_embed_rows(trace_ctx* c, const int32_t* ids, int n_ids, const int32_t* time_rows, int n_time,
                                const int32_t* score_rows, int n_score, void* embeds_out, void* stream) {
    if (!c || !c->finalized) return fail(TRACE_ERR_STATE, "context not finalized");
    if (!ids || n_ids < 1) return fail(TRACE_ERR_ARG, "bad ids");
    if (n_ids > c->max_ctx) return fail(TRACE_ERR_ARG, "more rows than max_ctx");
    for (int i = 0; i < n_ids; ++i)
        if (ids[i] == -201 || ids[i] == -200) return fail(TRACE_ERR_ARG, "a <video> placeholder among the ids: trace_embed_rows takes rows that hold no video");
    return splice_rows(c, ids, n_ids, time_rows, n_time, score_rows, n_score, n_ids, embeds_out, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------ frame preprocessing
// Pillow's Resample.c precompute_coeffs + normalize_coeffs_8bpc for the BICUBIC filter, in its operation order (double).
#pragma clang fp contract(off)
static double pil_bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
static int pil_coeffs(int in_size, int out_size, std::vector<int32_t>& bounds, std::vector<int32_t>& kk) {
    double scale, filterscale;
    scale = filterscale = (double)in_size / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 2.0 * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    bounds.assign((size_t)out_size * 2, 0);
    kk.assign((size_t)out_size * ksize, 0);
    std::vector<double> w(ksize);
    const double ss = 1.0 / filterscale;
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        for (int x = 0; x < xmax; ++x) { w[x] = pil_bicubic((x + xmin - center + 0.5) * ss); ww += w[x]; }
        for (int x = 0; x < xmax; ++x) {
            const double k = ww != 0.0 ? w[x] / ww : w[x];
            kk[(size_t)xx * ksize + x] = k < 0 ? (int)(-0.5 + k * (1 << 22)) : (int)(0.5 + k * (1 << 22));
        }
        bounds[2 * xx] = xmin; bounds[2 * xx + 1] = xmax;
    }
    return ksize;
}

extern "C" int trace_preprocess_frames(trace_ctx* c, const void* frames_u8, int T, int H, int W, int pad_to_square,
                                       const float* image_mean, const float* image_std, void* out, int out_dtype, void* stream) {
    if (!c) return fail(TRACE_ERR_ARG, "null ctx");
    if (!frames_u8 || !out || !image_mean || !image_std || T < 1 || H < 1 || W < 1 || (out_dtype != 0 && out_dtype != 1))
        return fail(TRACE_ERR_ARG, "bad preprocess arguments");
    hipStream_t s = (hipStream_t)stream;
    const int S = c->c.v_image;
    // geometry: expand2square (mm_utils.py:259-270), shortest edge -> S (HF get_resize_output_image_size), centre crop
    int PH = H, PW = W, y0 = 0, x0 = 0;
    if (pad_to_square && H != W) {
        PH = PW = H > W ? H : W;
        if (W > H) y0 = (W - H) / 2; else x0 = (H - W) / 2;
    }
    int nh, nw;
    if (PW <= PH) { nw = S; nh = (int)((double)((long)S * PH) / (double)PW); }
    else { nh = S; nw = (int)((double)((long)S * PW) / (double)PH); }
    const int top = (nh - S) / 2, left = (nw - S) / 2;
    std::vector<int32_t> bh, kh, bv, kv;
    const int ksh = pil_coeffs(PW, nw, bh, kh), ksv = pil_coeffs(PH, nh, bv, kv);
    const int row_first = bv[2 * top], row_last = bv[2 * (top + S - 1)] + bv[2 * (top + S - 1) + 1];
    const int nrows = row_last - row_first;
    // device tables: cropped columns / rows only; vertical bounds relative to the first staged row
    std::vector<int32_t> tab((size_t)S * 2 * 2 + (size_t)S * (ksh + ksv));
    int32_t* tbh = tab.data(); int32_t* tbv = tbh + 2 * S; int32_t* tkh = tbv + 2 * S; int32_t* tkv = tkh + (size_t)S * ksh;
    for (int j = 0; j < S; ++j) {
        tbh[2 * j] = bh[2 * (left + j)]; tbh[2 * j + 1] = bh[2 * (left + j) + 1];
        tbv[2 * j] = bv[2 * (top + j)] - row_first; tbv[2 * j + 1] = bv[2 * (top + j) + 1];
        memcpy(tkh + (size_t)j * ksh, kh.data() + (size_t)(left + j) * ksh, (size_t)ksh * 4);
        memcpy(tkv + (size_t)j * ksv, kv.data() + (size_t)(top + j) * ksv, (size_t)ksv * 4);
    }
    // rescale + normalise of an 8-bit value, in the reference's arithmetic: float32(float64(u) * (1/255)), (x - mean) / std
    std::vector<float> lut(3 * 256);
    uint32_t bg = 0;
    for (int ch = 0; ch < 3; ++ch) {
        for (int u = 0; u < 256; ++u) {
            const float x = (float)((double)u * (1.0 / 255));
            lut[ch * 256 + u] = (x - image_mean[ch]) / image_std[ch];
        }
        bg |= (uint32_t)((int)(image_mean[ch] * 255) & 255) << (8 * ch);       // int(x*255), mm_utils.py:457
    }
    const size_t tab_bytes = tab.size() * 4, lut_bytes = lut.size() * 4, tmp_bytes = (size_t)T * nrows * S * 3;
    if (c->pp_bytes < tab_bytes + lut_bytes + tmp_bytes + 512) {
        HIPCHK(hipStreamSynchronize(s));
        if (c->pp_buf) hipFree(c->pp_buf);
        c->pp_bytes = tab_bytes + lut_bytes + tmp_bytes + 512;
        HIPCHK(hipMalloc(&c->pp_buf, c->pp_bytes));
    }
    char* base = (char*)c->pp_buf;
    int32_t* d_tab = (int32_t*)base;
    float* d_lut = (float*)(base + ((tab_bytes + 255) & ~(size_t)255));
    uint8_t* d_tmp = (uint8_t*)d_lut + ((lut_bytes + 255) & ~(size_t)255);
    HIPCHK(hipMemcpyAsync(d_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_lut, lut.data(), lut_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));                      // host vectors go out of scope below
    LCHK(launch_resize_h((const uint8_t*)frames_u8, T, H, W, y0, x0, bg, d_tab, d_tab + 4 * S, ksh, row_first, nrows, S, d_tmp, s));
    LCHK(launch_resize_v_norm(d_tmp, T, nrows, S, d_tab + 2 * S, d_tab + 4 * S + (size_t)S * ksh, ksv, d_lut, out, out_dtype, s));
    return TRACE_OK;
}

// ------------------------------------------------------------------------------------------------ LLM prefill
// nb equal-length sequences laid end to end in pX (rows [b*L, (b+1)*L)) -> slots slot0 .. slot0+nb-1.  Two 1967-row
// prompts give the GEMMs M = 3934: 16 row tiles fill the 256x256 tile grid in whole rounds (gate|up 1792 tiles = 7.0
// rounds instead of 896 = 3.5) and o-proj / down-proj reach the 256^2 kernel.
// past > 0 (trace_llm_prefill_append): every target slot already holds `past` rows; the nb x L new rows take positions past .. past + L - 1
// (RoPE, cache rows) and attend the cached rows 0 .. past - 1 as well: query row i of a prompt sees keys <= i + past.  Every kernel is the one
// the past == 0 call runs, every per-row sum in the same order: a row's bits do not depend on where the prompt was cut (tests/test_gpu_prefix_reuse.py).
// Under the e4m3 KV cache (c->kv8) the K / V^T the prefill kernels write and attend are ONE layer's 16-bit staging rows, prompt b in staging slot b:
// the same launches on other pointers, so a past == 0 prefill computes the bits of the 16-bit-cache context.  After a layer's attention kv8_pack moves rows
// past .. past + L - 1 into the cache; with past > 0 kv8_unpack first fills staging rows 0 .. past - 1 from it, so the new rows attend the QUANTISED past
// (what the decode steps will see) — deterministic, but not the bits of an uncut prefill.
static Kv8Cache kv8_layer(const trace_ctx* c, int l) {
    return Kv8Cache{c->k8cache + (size_t)l * c->layer_stride, c->v8cache + (size_t)l * c->layer_stride, c->kscache + (size_t)l * (c->layer_stride / c->HD),
                    c->vscache + (size_t)l * (c->layer_stride / c->HD), (long)c->slot_stride, (long)c->kv_head_stride, c->ctx_pad};
}
static int prefill_kv8_pack(trace_ctx* c, int l, int slot0, int nb, int L, int past, hipStream_t s) {
    return launch_kv8_pack(c->kv_stage_k + (size_t)past * c->HD, (long)c->slot_stride, (long)c->kv_head_stride, c->HD,
                           c->pQKV + (size_t)(c->NQ + c->NKV) * c->HD, (long)L * c->QKV, c->HD, c->QKV, kv8_layer(c, l), c->d_ident + slot0, past, L, nb, c->NKV, s);
}
// The rows of the row-major workspaces (pX, pH, pO, pACT, pQKV) that a stage reads and writes in place: rows first + i * mult, i < n.  A stage takes the
// pointers `first` rows in and mult x width as the leading dimensions.
struct PfRows { int first, n, mult; };
static int prefill_impl(trace_ctx* c, int slot0, int nb, int L, void* hidden_out, hipStream_t s, int past = 0) {
    const int H = c->H, I = c->I, HD = c->HD, QKV = c->QKV, M = nb * L;
    const int QW = c->NQ * HD, KVW = 2 * c->NKV * HD;  // the q and the k | v columns of a qkv row
    const int kslot0 = c->kv8 ? 0 : slot0;            // first K / V^T slot the layer's kernels use
    AttnArgs a{};
    a.q_bs = (long)L * QKV; a.q_hs = HD; a.q_rs = QKV;
    a.k_bs = (long)c->slot_stride; a.k_hs = (long)c->kv_head_stride; a.k_rs = HD;
    a.v_bs = (long)c->slot_stride; a.v_hs = (long)c->kv_head_stride; a.v_rs = c->ctx_pad;      // V^T straight from the cache
    a.o_bs = (long)L * H; a.o_hs = HD; a.o_rs = H;
    a.nkv_rows = past + L; a.batch = nb; a.heads = c->NQ; a.kv_heads = c->NKV;
    a.scale = 1.0f / sqrtf((float)HD); a.causal = 1;
    for (int l = 0; l < c->NL; ++l) {
        const LlmLayer& W = c->llm[l];
        auto P = layer_projs(W, H, I, QKV);           // the row-major copies: 16-bit, or e4m3 + row scales
        if (c->w4)            // this layer's four projections as 16-bit rows (exactly the weights the decode GEMVs widen); the GEMMs below run on them unchanged
            for (int p = 0; p < 4; ++p) {
                LCHK(launch_dequant_w4(P[p].w4c, P[p].w4e, c->w4_row[p], P[p].K, P[p].N, P[p].K, s));
                P[p].w = c->w4_row[p];
            }
        // Projection p over n rows: C = A W^T, + R when given (R lies where C does: ldr = ldc).  cols > 0: only the output columns col0 .. col0 + cols - 1.
        auto proj = [&](int p, const bf16_t* A, int lda, bf16_t* C, int ldc, const bf16_t* R, int n, int epi, int col0 = 0, int cols = 0) {
            const int N = cols ? cols : P[p].N, K = P[p].K, ldr = R ? ldc : 0;
            if (c->fp8) return gemm_fp8(c, A, lda, P[p].w8 + (size_t)col0 * K, P[p].sw + col0, C, ldc, R, ldr, n, N, K, epi, s);
            return gemm(A, lda, P[p].w + (size_t)col0 * K, K, C, ldc, nullptr, R, ldr, n, N, K, epi, s);
        };
        bf16_t* kc = c->kv8 ? c->kv_stage_k : c->kcache + (size_t)l * c->layer_stride;
        bf16_t* vc = c->kv8 ? c->kv_stage_v : c->vcache + (size_t)l * c->layer_stride;
        if (c->kv8 && past > 0)
            LCHK(launch_kv8_unpack(kv8_layer(c, l), c->d_ident + slot0, kc, vc, (long)c->slot_stride, (long)c->kv_head_stride, c->ctx_pad, past, nb, c->NKV, s));
        LCHK(launch_rmsnorm(c->pX, H, c->pH, H, W.rms1, M, H, c->c.rms_eps, s));
        // Round 6: the LAST decoder layer of a prefill whose caller does not ask for the hidden rows.  What is consumed afterwards is the layer's K / V
        // rows of every position (the cache) and the final hidden state of each prompt's LAST row only (the reference computes all L rows of
        // everything, trace_mistral.py:190-200, and then uses logits[:, -1]) — so: the k | v slice of the qkv projection over all M rows, and q,
        // attention, o-proj and the MLP for the nb last rows, on the same kernels reading / writing those rows in place (row stride L x width).
        // Same MFMA tile kernels, same K order, same epilogues: bit-identical to the full layer (tests/test_gpu_parity.py), ~3 % of a prefill saved.
        // In the terms of this body the shortcut is a row set {L - 1, nb, L} for everything after the cache write, and a qkv projection split in two.
        // (The e4m3 weight paths do not take it — proj would serve them, the condition keeps them out.)
        const bool shortcut = g_tune.prefill_last_rows && l == c->NL - 1 && !hidden_out && !c->fp8 && L > 1;
        const PfRows r = shortcut ? PfRows{L - 1, nb, L} : PfRows{0, M, 1};
        const size_t r0 = (size_t)r.first;
        const int ldH = r.mult * H, ldI = r.mult * I, ldQ = r.mult * QKV;
        if (shortcut) {       // the one place where the shortcut is more than a row set: k | v for every row, q for the row set
            TRY(proj(0, c->pH, H, c->pQKV + QW, QKV, nullptr, M, EPI_NONE, QW, KVW));
            TRY(proj(0, c->pH + r0 * H, ldH, c->pQKV + r0 * QKV, ldQ, nullptr, r.n, EPI_NONE, 0, QW));
        } else TRY(proj(0, c->pH, H, c->pQKV, QKV, nullptr, M, EPI_NONE));
        // cache write and attend.  q and k rotated, k into the cache (under the shortcut this also rotates the stale q of the other rows: 10 us, nobody reads them)
        LCHK(launch_rope_kv(c->pQKV, QKV, kc, nullptr, (long)c->slot_stride, (long)c->kv_head_stride, nullptr, nullptr, kslot0, past, M,
                            c->NQ, c->NKV, HD, c->rope_cos, c->rope_sin, L, s));
        // V goes into the cache transposed ([kvh][hd][ctx_pad]; positions past+L..Lpad-1 are zero-filled, later overwritten)
        LCHK(launch_transpose_v(c->pQKV + (size_t)(c->NQ + c->NKV) * HD, (long)L * QKV, HD, QKV, vc + (size_t)kslot0 * c->slot_stride,
                                (long)c->slot_stride, (long)c->kv_head_stride, c->ctx_pad, L, HD, c->NKV, nb, s, 0, past));
        // the row set's queries against all past + L keys of their prompt (r.n / nb query rows a prompt: L, or the one row L - 1 — causal offset nkv - nq)
        a.Q = c->pQKV + r0 * QKV; a.O = c->pO + r0 * H; a.nq_rows = r.n / nb;
        a.K = kc + (size_t)kslot0 * c->slot_stride;
        a.V = vc + (size_t)kslot0 * c->slot_stride;
        LCHK(launch_attn_prefill(a, s));
        if (c->kv8) LCHK(prefill_kv8_pack(c, l, slot0, nb, L, past, s));
        // tail over the row set: o-proj + residual, norm, gate|up SwiGLU, down + residual
        bf16_t *x = c->pX + r0 * H, *h = c->pH + r0 * H, *act = c->pACT + r0 * I;
        TRY(proj(1, c->pO + r0 * H, ldH, x, ldH, x, r.n, EPI_RESIDUAL));
        LCHK(launch_rmsnorm(x, ldH, h, ldH, W.rms2, r.n, H, c->c.rms_eps, s));
        TRY(proj(2, h, ldH, act, ldI, nullptr, r.n, EPI_SWIGLU));
        TRY(proj(3, act, ldI, x, ldH, x, r.n, EPI_RESIDUAL));
    }
    if (hidden_out) LCHK(launch_rmsnorm(c->pX, H, (bf16_t*)hidden_out, H, c->final_norm, M, H, c->c.rms_eps, s));
    for (int b = 0; b < nb; ++b) {
        LCHK(launch_rmsnorm(c->pX + ((size_t)b * L + L - 1) * H, H, c->xlast + (size_t)(slot0 + b) * H, H, c->final_norm, 1, H,
                            c->c.rms_eps, s));
        c->slot_len[slot0 + b] = past + L;
    }
    return TRACE_OK;
}

// ---- the entry path: all six calls that prefill come through prefill_entry ----
// The argument rules of a pass: n slots that hold at least `past` rows each (a prompt prefix prefilled or copied there earlier; a whole prompt is
// past == 0) take L new rows per slot.  (trace_llm_score_append has no hidden_out and passes NULL;
// have >= 0: the rows every slot WILL hold when the pass runs, for a caller that fills them first)
static int append_check(trace_ctx* c, int slot0, int n, int past, const void* const* embeds, int L, const void* hidden_out, int have = -1) {
    if (!c || !c->finalized) return fail(TRACE_ERR_STATE, "context not finalized");
    if (n < 1 || n > PF_MAX_N || slot0 < 0 || slot0 + n > c->max_B) return fail(TRACE_ERR_ARG, "bad slot / n");
    if (L < 1 || past < 0) return fail(TRACE_ERR_ARG, "bad L / past");
    if ((long)past + L > c->max_ctx) return fail(TRACE_ERR_ARG, "past + L exceeds max_ctx");
    if ((size_t)n * L > pf_rows(c->max_ctx)) return fail(TRACE_ERR_ARG, "n x L exceeds the prefill workspace (max(4 max_ctx, min(8192, 8 max_ctx)) rows)");
    if (!embeds && n != 1) return fail(TRACE_ERR_ARG, "the internal embedding buffer holds one prompt: embeds may be NULL with n == 1 only");
    if (hidden_out && n != 1) return fail(TRACE_ERR_ARG, "hidden_out with n == 1 only");
    for (int i = 0; i < n; ++i) {
        if (embeds && !embeds[i]) return fail(TRACE_ERR_ARG, "null embeds");
        if (past > (have >= 0 ? have : c->slot_len[slot0 + i])) return fail(TRACE_ERR_STATE, "past exceeds the rows the slot holds");
    }
    return TRACE_OK;
}
// append_check, then `before` (what a caller has left to refuse or to enqueue ahead of the pass: trace_llm_prefill_shared's fan-out of the prefix,
// trace_llm_score_append's heads and ids), then the n prompts' new rows end to end into pX (embeds == NULL: the internal buffer already holds them), then
// prefill_impl.  Everything is checked before the first launch.  rows_hidden: every row's final-norm hidden state is kept in pH, which is free once
// the last layer is done (any n; hidden_out is the caller's buffer and n == 1 only).
static int nothing_before() { return TRACE_OK; }
template <class Before = int (*)()>
static int prefill_entry(trace_ctx* c, int slot0, int n, int past, const void* const* embeds, int L, void* hidden_out, void* stream, int have = -1,
                         bool rows_hidden = false, Before before = nothing_before) {
    TRY(append_check(c, slot0, n, past, embeds, L, hidden_out, have));
    TRY(before());
    hipStream_t s = (hipStream_t)stream;
    if (embeds)
        for (int i = 0; i < n; ++i) HIPCHK(hipMemcpyAsync(c->pX + (size_t)i * L * c->H, embeds[i], (size_t)L * c->H * 2, hipMemcpyDeviceToDevice, s));
    return prefill_impl(c, slot0, n, L, rows_hidden ? c->pH : hidden_out, s, past);
}

extern "C" int trace_llm_prefill(trace_ctx* c, int slot, const void* embeds, int L, void* hidden_out, void* stream) {
    return prefill_entry(c, slot, 1, 0, embeds ? &embeds : nullptr, L, hidden_out, stream);
}

extern "C" int trace_llm_prefill_pair(trace_ctx* c, int slot0, const void* embeds0, const void* embeds1, int L, void* stream) {
    const void* embeds[2] = {embeds0, embeds1};
    return prefill_entry(c, slot0, 2, 0, embeds, L, nullptr, stream);
}

// n <= 8 prompts of EQUAL spliced length in one pass while n x L <= max(4 max_ctx, min(8192, 8 max_ctx)) rows (the prefill workspaces) -> KV slots slot0 .. slot0 + n - 1.  Four 1967-row prompts give the GEMMs M = 7868 = 31 row tiles:
// qkv 744 tiles = 2.9 rounds of the 256 CUs (a pair: 384 = 1.5 rounds, a quarter of the second round's CUs idle), o / down 496 = 1.94, gate|up 13.6
extern "C" int trace_llm_prefill_multi(trace_ctx* c, int slot0, const void* const* embeds, int n, int L, void* stream) {
    if (c && c->finalized && !embeds) return fail(TRACE_ERR_ARG, "null embeds");      // (the internal buffer is trace_llm_prefill's and trace_llm_prefill_append's to use)
    return prefill_entry(c, slot0, n, 0, embeds, L, nullptr, stream);
}

// Continue n slots that hold at least `past` rows each with L new rows per slot: what trace_llm_prefill_multi is for whole prompts.
extern "C" int trace_llm_prefill_append(trace_ctx* c, int slot0, int n, int past, const void* const* embeds, int L, void* hidden_out, void* stream) {
    return prefill_entry(c, slot0, n, past, embeds, L, hidden_out, stream);
}

// Rows [0, rows) of every layer's K and V^T from one slot to n others (launch_kv_copy, KV_COPY_MAX destinations per launch).  A copy of ALL the
// source's rows also takes its last-position hidden row, so the destination can be decoded from as the source can.
extern "C" int trace_kv_copy(trace_ctx* c, int src_slot, const int32_t* dst_slots, int n, int rows, void* stream) {
    if (!c || !c->finalized) return fail(TRACE_ERR_STATE, "context not finalized");
    if (!dst_slots || n < 1 || n > c->max_B) return fail(TRACE_ERR_ARG, "bad dst_slots / n");
    if (src_slot < 0 || src_slot >= c->max_B) return fail(TRACE_ERR_ARG, "source slot out of range");
    if (rows < 1) return fail(TRACE_ERR_ARG, "bad rows");
    if (rows > c->slot_len[src_slot]) return fail(TRACE_ERR_STATE, "rows exceeds the rows the source slot holds");
    for (int i = 0; i < n; ++i) {
        if (dst_slots[i] < 0 || dst_slots[i] >= c->max_B) return fail(TRACE_ERR_ARG, "destination slot out of range");
        if (dst_slots[i] == src_slot) return fail(TRACE_ERR_ARG, "the source slot is among the destinations");
    }
    hipStream_t s = (hipStream_t)stream;
    for (int i0 = 0; i0 < n; i0 += KV_COPY_MAX) {
        KvCopyDst d{};
        d.n = std::min(KV_COPY_MAX, n - i0);
        for (int i = 0; i < d.n; ++i) d.slot[i] = dst_slots[i0 + i];
        if (c->kv8) { LCHK(launch_kv8_copy(kv8_layer(c, 0), (long)c->layer_stride, c->NL, c->NKV, src_slot, d, rows, s)); continue; }
        LCHK(launch_kv_copy(c->kcache, c->vcache, (long)c->layer_stride, (long)c->slot_stride, (long)c->kv_head_stride, c->ctx_pad, c->HD, c->NL,
                            c->NKV, src_slot, d, rows, s));
    }
    for (int i = 0; i < n; ++i) {
        if (rows == c->slot_len[src_slot])
            HIPCHK(hipMemcpyAsync(c->xlast + (size_t)dst_slots[i] * c->H, c->xlast + (size_t)src_slot * c->H, (size_t)c->H * 2, hipMemcpyDeviceToDevice, s));
        c->slot_len[dst_slots[i]] = rows;
    }
    return TRACE_OK;
}

// A run of a batch that shares its first `past` prompt rows: slot src_slot holds them (prefilled once for the batch); they are copied to the run's other
// slots (trace_kv_copy's launches) and the n prompts continue with their own L rows (trace_llm_prefill_append's body) — one call per run, everything checked
// before the first launch.  src_slot may be one of the run's slots (it is, in the batch's first run) and may hold more than `past` rows (in the later ones).
extern "C" int trace_llm_prefill_shared(trace_ctx* c, int src_slot, int slot0, int n, int past, const void* const* embeds, int L, void* stream) {
    if (!c || !c->finalized) return fail(TRACE_ERR_STATE, "context not finalized");
    if (c->kv8 || c->fp8) return fail(TRACE_ERR_STATE, "a shared prefix needs the 16-bit KV cache and 16-bit weights (a continuation is bit-identical there only)");
    if (src_slot < 0 || src_slot >= c->max_B || past < 1) return fail(TRACE_ERR_ARG, "bad source slot / past");
    if (past > c->slot_len[src_slot]) return fail(TRACE_ERR_STATE, "past exceeds the rows the source slot holds");
    if (!embeds) return fail(TRACE_ERR_ARG, "null embeds");
    return prefill_entry(c, slot0, n, past, embeds, L, nullptr, stream, past, false, [&] {
        int32_t dst[PF_MAX_N];
        int m = 0;
        for (int i = 0; i < n; ++i) if (slot0 + i != src_slot) dst[m++] = slot0 + i;
        return m ? trace_kv_copy(c, src_slot, dst, m, past, stream) : (int)TRACE_OK;
    });
}

// masked logits of R final-norm hidden rows under ONE head: what forward() returns for every position of a sequence
// (trace_mistral.py:190-252) — the decode loop itself only ever needs the last row (trace_decode_begin / _steps)
extern "C" int trace_llm_head_logits(trace_ctx* c, const void* hidden, int R, int head, float* logits_out, void* stream) {
    if (!c || !c->finalized) return fail(TRACE_ERR_STATE, "context not finalized");
    if (!hidden || !logits_out || R < 1) return fail(TRACE_ERR_ARG, "bad hidden / logits_out / R");
    if (head < 0 || head > 2) return fail(TRACE_ERR_ARG, "head must be 0, 1 or 2");
    hipStream_t s = (hipStream_t)stream;
    const bf16_t* x = (const bf16_t*)hidden;
    for (int r0 = 0; r0 < R; r0 += SK_ROWS)
        LCHK(launch_head_logits(x + (size_t)r0 * c->H, c->H, c->wheads, c->H, c->d_heads_tmp + head * SK_ROWS, c->V, c->Tv, c->Sv, c->hl_val, c->hl_idx,
                                logits_out + (size_t)r0 * c->NV, std::min(SK_ROWS, R - r0), s));
    return TRACE_OK;
}

// ------------------------------------------------------------------------------------------------ decode
// The rows a tail launch works on.  The batch: rows [0, B), the shared counter d_step[0..1], every row's origin d_step0.  The rows an admission
// appends (trace_decode_admit): rows [r0, r0 + n) as a batch of their own, with the spare counter pair d_step[2..3] (which the admission zeroes
// first) and no origin, so the selection they run is their step 0 while the shared counter and the rows in front of r0 are not touched.
struct TailRows { int r0, n; };
static StepState step_state(trace_ctx* c, TailRows t = {0, 0}) {
    StepState st{};
    const size_t r0 = (size_t)t.r0;
    st.heads = c->d_heads + r0; st.pos = c->d_pos + r0; st.done = c->d_done + r0; st.out_ids = c->d_out_ids + r0 * c->max_new; st.out_len = c->d_out_len + r0;
    st.step = t.r0 ? c->d_step + 2 : c->d_step; st.forced = c->d_forced + r0 * c->max_new; st.params = c->d_params; st.row_id = c->d_row_id + r0;
    st.step0 = t.r0 ? nullptr : c->d_step0;
    if (c->armed.per_row) { st.row_sp = c->d_row_sp + r0; st.row_lp = c->d_row_lp + r0; st.row_max_new = c->d_row_max + r0; }
    return st;
}

// Everything the batch holds per row, each column named ONCE, in the order retire.hip moves them (RetireArgs: 7 of one int, 3 of max_new ints, the 3
// per-row params, x): the device base as ints, the ints a row, whether the armed mode has the column, the host mirror of the SEATED values (h_pos0 keeps
// the prefill length: the device column advances).  seat_write, trace_decode_retire and trace_debug_decode_rows walk it: a new one-int column is one
// line here before out_ids (RETIRE_SMALL + 1 in kernels.h) and its seat value at the same place in seat_write.
struct RowCol { const char* name; int32_t* dev; int ints; bool on; void* host; };
constexpr int N_COLS = RETIRE_SMALL + 7;
static std::array<RowCol, N_COLS> row_cols(trace_ctx* c) {
    const int W = c->max_new, SP = sizeof(SampleParams) / 4, LP = sizeof(LogitsParams) / 4;
    const bool pr = c->armed.per_row;
    auto I = [](auto* p) { return reinterpret_cast<int32_t*>(p); };
    return {{{"slots", c->d_slots, 1, true, c->h_slots}, {"pos", c->d_pos, 1, true, c->h_pos0}, {"heads", c->d_heads, 1, true, nullptr},
             {"done", c->d_done, 1, true, nullptr}, {"out_len", c->d_out_len, 1, true, nullptr}, {"row_id", c->d_row_id, 1, true, nullptr},
             {"step0", c->d_step0, 1, true, c->h_step0},
             {"out_ids", c->d_out_ids, W, true, nullptr}, {"forced", c->d_forced, W, true, nullptr}, {"logprobs", I(c->d_logprobs), W, c->armed.logprobs, nullptr},
             {"row_sp", I(c->d_row_sp), SP, pr, c->h_row_sp}, {"row_lp", I(c->d_row_lp), LP, pr, c->h_row_lp}, {"row_max", c->d_row_max, 1, pr, c->h_row_max},
             {"x", I(c->dX), c->H / 2, true, nullptr}}};
}

static int head_only(trace_ctx* c, const bf16_t* xn, float* logits_out, hipStream_t s, TailRows t) {
    LCHK(launch_head_logits(xn, c->H, c->wheads, c->H, c->d_heads + t.r0, c->V, c->Tv, c->Sv, c->part_val + (size_t)t.r0 * c->ntiles,
                            c->part_idx + (size_t)t.r0 * c->ntiles, logits_out, t.n, s));
    return TRACE_OK;
}
// the selection in one of its forms; `rows`: the masked logits SELECT_SAMPLE / SELECT_ROW read (null for SELECT_TILES, which reads the tile partials)
static int select_only(trace_ctx* c, int form, const float* rows, int advance, hipStream_t s, TailRows t = {0, 0}) {
    if (!t.n) t.n = c->B;
    LCHK(launch_select(form, c->part_val + (size_t)t.r0 * c->ntiles, c->part_idx + (size_t)t.r0 * c->ntiles, rows, form == SELECT_SAMPLE ? c->d_sparams : nullptr,
                       step_state(c, t), c->embed, c->time_tab, c->score_tab, c->sync_row, c->dX + (size_t)t.r0 * c->H, c->H, t.n, c->H, c->V, c->Tv, c->Sv,
                       advance, s, c->armed.stop ? c->d_ctab : nullptr));
    return TRACE_OK;
}
// xn / logits_out: the first of the t.n rows
static int head_and_select(trace_ctx* c, const bf16_t* xn, int advance, float* logits_out, hipStream_t s, TailRows t = {0, 0}) {
    const TailMode m = c->armed;
    if (!t.n) t.n = c->B;
    const size_t lg0 = (size_t)t.r0 * c->NV;
    // 1. the head: tile partials, and the raw masked rows into the caller's logits_out, else d_slog when anything armed will read them, else nowhere
    float* raw = !logits_out && m.index() ? c->d_slog + lg0 : logits_out;
    TRY(head_only(c, xn, raw, s, t));
    // 2. host-select mode ends here: the host picks the token and calls trace_decode_feed
    if (c->host_mode) return TRACE_OK;
    // 3. logits processors and the ban rules of the constraints: the raw rows -> d_plog (raw stays as it is for step 5)
    if (m.process) LCHK(launch_step_logits_process(raw, step_state(c, t), t.n, c->V, c->Tv, c->Sv, c->d_lgparams, c->d_plog + lg0, s, c->d_ctab));
    // 4. the selection: a draw from the rows, the arg-max over a processed row, or the arg-max over the tile partials (they describe the raw row);
    //    with stop sequences armed, the instantiation that matches them against the recorded ids
    //    a batch with per-row params: the form that takes either by the row's own params, over the processed rows where any row's processors or the
    //    batch's ban rules are armed (m.process, decided at begin / admit from the host copy), else over the raw ones
    const int form = m.per_row ? SELECT_PER_ROW : m.sample ? SELECT_SAMPLE : m.process ? SELECT_ROW : SELECT_TILES;
    TRY(select_only(c, form, form == SELECT_TILES ? nullptr : m.process ? c->d_plog + lg0 : raw, advance, s, t));
    // 5. the log-probability of the token just recorded (it reads out_ids / out_len / the advanced step counter), on the raw rows
    if (m.logprobs) LCHK(launch_step_logprob(raw, step_state(c, t), t.n, c->V, c->Tv, c->Sv, c->d_logprobs + (size_t)t.r0 * c->max_new, s));
    return TRACE_OK;
}

// Everything one decode step decides before it launches.  Pure: the tuning values come as an argument, nothing is kept between steps, and the only HIP
// call behind it is the GEMV plan's CU count, asked once per process.  trace_op_decode_route shows it to host tests.  scheme: trace_config::llm_weights_fp8, or 3 for w4 weights.
//   step (= prof[8]): 3 wide above SKINNY_ROWS and, on bf16 weights, from decode.wide_min_rows; 2 fused up to decode.fuse_norm_rows on bf16 weights where
//     both fused-norm GEMVs take the shape; 1 skinny otherwise.
//   qkv_finish: RoPE + cache append as a launch of its own instead of the attention's prologue (decode.unfused_qkv, wide: decode.wide_fuse_qkv).
//   ks_*: K-chunks of the qkv / o / gate|up / down partial rows (the wide step's gate|up GEMM has none: 0).
//   nsplit, the attention's context split: ~256-320 workgroups (8 kv heads x B x nsplit) fill the CUs; more splits only add partial-result traffic and
//     ticket latency (measured, ctx 2100: B=1 16 splits 10.4 us, B=4 8 -> 13 us, B=16 2 -> 26 us, B=32 1 -> 45 us; B=32 with 16 splits: 79 us).
//     attn.decode.nsplit > 0 forces the number (A/B).
struct DecodeRoute { int step; SkinnyKind kind; bool qkv_finish; int ks_q, ks_o, ks_g, ks_d, nsplit; };
static DecodeRoute decode_route(int B, int scheme, int H, int I, int QKV, const Tuning& t) {
    DecodeRoute r{};
    const bool quant = scheme != 0;                // quantised weights of either format (3 = w4: routed as the weight-only fp8 scheme is, on its own kind of GEMV)
    r.kind = !quant ? SK_BF16 : scheme == 3 ? SK_W4A16 : scheme == 2 ? SK_W8A16 : SK_W8A8;
    if (B > SKINNY_ROWS || (B >= t.decode_wide_min_rows && !quant)) r.step = 3;
    else r.step = B <= t.decode_fuse_norm_rows && !quant && skinny_fused_norm_ok(QKV, H, B) && skinny_fused_norm_ok(2 * I, H, B) ? 2 : 1;
    r.qkv_finish = r.step == 3 ? !t.decode_wide_fuse_qkv : r.step == 1 && (t.decode_unfused_qkv == 1 || (t.decode_unfused_qkv == 0 && B >= 32));
    auto ks = [&](int N, int K) { return r.step == 3 ? gemm_partial_ks(N, K, t) : skinny_ks(r.kind, N, K, EPI_PARTIAL, B); };
    r.ks_q = ks(QKV, H); r.ks_o = ks(H, H); r.ks_g = r.step == 3 ? 0 : ks(2 * I, H); r.ks_d = ks(H, I);
    r.nsplit = t.attn_decode_nsplit > 0 ? t.attn_decode_nsplit : std::max(1, std::min(16, (40 + B / 2) / B));
    return r;
}

// Roofline probe (profile == 2): HIP events around ONE launch per step, layer 0's dominant kernel, for the scope this object lives in; `kind` says
// which launch took the bracket (prof[8]).  Eager launches only: event-record nodes captured into a hipGraph do not yield usable timestamps on ROCm 7.2.
struct StepBracket {
    hipEvent_t e1 = nullptr; hipStream_t s;
    StepBracket(trace_ctx* c, int l, int kind, hipStream_t s_, int bit = 2) : s(s_) {
        if (l != 0 || c->profile != 2 || !(c->bracket_mask & bit) || s == c->cap_stream || c->kev_used + 2 > (int)c->kev.size()) return;
        hipEventRecord(c->kev[c->kev_used], s);
        e1 = c->kev[c->kev_used + 1]; c->kev_used += 2; c->bracket_kind = kind;
    }
    ~StepBracket() { if (e1) hipEventRecord(e1, s); }
};
// algorithmic bytes of one layer's decode attention in the current step: the K + V rows of every sequence, 16-bit, or e4m3 + two scales
static double attn_kv_bytes(const trace_ctx* c) {
    return (double)(c->pos_sum + (long)c->B * (c->step_in_call + 1)) * c->NKV * (c->kv8 ? 2 * c->HD + 8 : c->HD * 2 * 2);
}

// The decode attention of layer l.  Without r.qkv_finish its prologue sums the qkv partial rows part [r.ks_q][SK_ROWS][QKV], applies RoPE and appends
// k / v to the cache; otherwise dQKV holds ready q rows and the cache the new row (qkv_finish_layer ran).
static int attn_decode_layer(trace_ctx* c, int l, const DecodeRoute& r, const float* part, hipStream_t s) {
    const bool fused = !r.qkv_finish;
    StepBracket br(c, l, 3, s, 4);                  // bracket bit 2: this launch in whichever step body runs (with its fused prologue, where it has one)
    if (br.e1) c->kbytes_sum += attn_kv_bytes(c);
    if (c->kv8)       // no fused prologue over the e4m3 cache: decode_step sets r.qkv_finish
        return fused ? TRACE_ERR_STATE
                     : launch_attn_decode_kv8(c->dQKV, c->QKV, kv8_layer(c, l), c->d_slots, c->d_pos, c->dO, c->H, c->attn_ws, c->tickets, c->B, c->NQ, c->NKV,
                                              c->HD, r.nsplit, 1.0f / sqrtf((float)c->HD), s);
    return launch_attn_decode(c->dQKV, c->QKV, c->kcache + (size_t)l * c->layer_stride, c->vcache + (size_t)l * c->layer_stride, (long)c->slot_stride,
                              (long)c->kv_head_stride, c->ctx_pad, c->d_slots, c->d_pos, c->dO, c->H, c->attn_ws, c->tickets, c->B, c->NQ, c->NKV, c->HD,
                              r.nsplit, 1.0f / sqrtf((float)c->HD), fused ? 1 : 0, fused ? c->rope_cos : nullptr, fused ? c->rope_sin : nullptr,
                              fused ? part : nullptr, fused ? r.ks_q : 0, s, c->sh_slot, c->sh_rows);
}
// that prologue as a launch of its own: the qkv partial rows in sk_ws -> roped q rows in dQKV, k / v of layer l appended
static int qkv_finish_layer(trace_ctx* c, int l, int ks, hipStream_t s, const float* part = nullptr) {
    if (!part) part = c->sk_ws;
    StepBracket br(c, l, 4, s, 8);                  // bracket bit 3: the append launch
    if (c->kv8) return launch_qkv_finish_kv8(part, ks, c->QKV, c->dQKV, kv8_layer(c, l), c->d_slots, c->d_pos, c->B, c->NQ, c->NKV, c->rope_cos, c->rope_sin, s);
    return launch_qkv_finish(part, ks, c->QKV, c->dQKV, c->kcache + (size_t)l * c->layer_stride, c->vcache + (size_t)l * c->layer_stride,
                             (long)c->slot_stride, (long)c->kv_head_stride, c->ctx_pad, c->d_slots, c->d_pos, c->B, c->NQ, c->NKV, c->rope_cos, c->rope_sin, s);
}

// One decode step for 1..4 sequences (the reference drivers' own call shape is 1): the two "sum the partial rows + residual -> new residual, RMSNorm"
// kernels of a layer are folded into the GEMVs that consume their output (decode.hip, SkinnyPro), and (round 4) the SwiGLU combine into the down
// GEMV — 4 launches per layer instead of 7:
//   qkv GEMV [sums the previous layer's down partials + residual, input norm] -> attention (RoPE / append / attention) -> o GEMV
//   -> gate|up GEMV [sums the o partials + residual, post-attention norm] -> down GEMV [sums the gate|up partials, SwiGLU]
// Partial rows alternate between sk_ws (written by o / down, read by the fused GEMVs) and sk_ws2 (written by the fused GEMVs, read by the attention /
// the combine); the residual rows alternate between dX and dX2 (a fused GEMV reads one and writes the other: its workgroups all read the whole row).
static int decode_step_fused(trace_ctx* c, const DecodeRoute& r, float* logits_out, hipStream_t s) {
    const int H = c->H, I = c->I, QKV = c->QKV, B = c->B;
    bf16_t *xa = c->dX, *xb = c->dX2;             // current / next residual rows
    for (int l = 0; l < c->NL; ++l) {
        const LlmLayer& W = c->llm[l];
        const auto P = layer_projs(W, H, I, QKV);      // the bf16 tile copies
        LCHK(launch_skinny_gemm_fused_norm(l ? c->sk_ws : nullptr, l ? r.ks_d : 0, xa, H, xb, H, W.rms1, c->c.rms_eps, P[0].wd, B, QKV, H, c->sk_ws2,
                                           c->sk_ws_floats, s));
        std::swap(xa, xb);
        if (r.qkv_finish) LCHK(qkv_finish_layer(c, l, r.ks_q, s, c->sk_ws2));      // (the e4m3 KV cache only: this step's 16-bit form always fuses the append)
        LCHK(attn_decode_layer(c, l, r, c->sk_ws2, s));
        LCHK(launch_skinny_gemm(c->dO, H, P[1].wd, H, nullptr, H, nullptr, 0, B, H, H, EPI_PARTIAL, 1, SKWS(c), s));
        {
            StepBracket br(c, l, 2, s);
            LCHK(launch_skinny_gemm_fused_norm(c->sk_ws, r.ks_o, xa, H, xb, H, W.rms2, c->c.rms_eps, P[2].wd, B, 2 * I, H, c->sk_ws2, c->sk_ws_floats, s));
        }
        std::swap(xa, xb);
        if (g_tune.decode_fuse_swiglu) {        // SwiGLU folded into the down GEMV's parking step (round 4, bit-identical to swiglu_combine + GEMV): 4 launches per layer
            LCHK(launch_skinny_gemm_fused_swiglu(c->sk_ws2, r.ks_g, P[3].wd, B, H, I, c->sk_ws, c->sk_ws_floats, s));
        } else {
            LCHK(launch_swiglu_combine(c->sk_ws2, r.ks_g, 2 * I, c->dACT, I, B, s));
            LCHK(launch_skinny_gemm(c->dACT, I, P[3].wd, I, nullptr, H, nullptr, 0, B, H, I, EPI_PARTIAL, 1, SKWS(c), s));
        }
    }
    // an even number of fused GEMVs: the residual rows are back in dX; the last layer's down partials + residual -> final norm -> heads
    LCHK(launch_add_rmsnorm(c->sk_ws, r.ks_d, xa, H, xa, H, c->final_norm, c->dH, H, B, H, c->c.rms_eps, s));
    return head_and_select(c, c->dH, 1, logits_out, s);
}

// One decode step on partial rows, in its two forms.  Every projection leaves fp32 k-chunk partial rows in sk_ws and its consumer sums them on load (an
// in-kernel merge costs 5-8 us of dependent round trips per GEMV): qkv -> attention (RoPE + cache append + attention) -> o -> [sum + residual -> new
// residual, RMSNorm] -> gate|up -> [sum, SwiGLU] -> down -> [sum + residual, next layer's / the final RMSNorm].
//   The GEMV step (r.step == 1), up to SKINNY_ROWS sequences on any kind of weights: a projection is a GEMV of the step's kind over the tile copies.
//   The wide step (r.step == 3), SKINNY_ROWS < B <= SK_ROWS sequences, 16-bit weights.  A GEMV that parks its activations in LDS cannot hold more than
//     64 rows x 1024 k, and its fp32 partial rows would grow with the row count; above 64 rows the projections are small-M GEMMs on the MFMA tile kernel
//     instead (gemm.hip, 128x128 tiles, weights from the row-major prefill copies, or the tile copies by decode.gemm_tiled), qkv / o / down cut along K
//     into gemm_partial_ks() chunks.  The weights (14 GB per step) are then streamed once per 128 tokens instead of once per 64: bytes per token
//     0.50 -> 0.39 GB at ctx ~2100, where the KV stream (0.27 GB per token) is the larger part.
// The two differ in two places, both below: what gate|up is, and which launch takes bracket bit 1.
static int decode_step_rows(trace_ctx* c, const DecodeRoute& r, float* logits_out, hipStream_t s) {
    const int H = c->H, I = c->I, QKV = c->QKV, B = c->B;
    const bool wide = r.step == 3;
    if (wide && (c->fp8 || c->w4)) return fail(TRACE_ERR_STATE, "the fp8 and w4 weight paths decode at most 64 sequences together");
    const int wt = g_tune.decode_gemm_tiled;
    const bool f8 = r.kind == SK_W8A8;               // activations quantised row-wise: dH arrives quantised (dH8 / dsh) from add_rmsnorm, only the step's first norm needs the quantiser
    const int ks[4] = {r.ks_q, r.ks_o, r.ks_g, r.ks_d};
    std::array<Proj, 4> P{};
    // Projection p of the layer in P, X [B, K] -> partial rows in sk_ws.  Wide: the partial GEMM.  Else the GEMV of the step's kind: the w4 tile copy (codes and
    // exponent bytes) with bf16 activations, the bf16 tile copy, or the e4m3 tile copy with bf16 activations (weight-only) or with activations quantised
    // first (quant_rows_fp8: [B, K] bf16 -> e4m3 + per-row scale; the normed rows dH are there already).
    auto proj = [&](int p, const bf16_t* X) -> int {
        const int N = P[p].N, K = P[p].K;
        if (wide) {
            GemmArgs g{X, K, (wt & 1) ? P[p].wd : P[p].w, K, nullptr, 0, nullptr, nullptr, 0, B, N, K, nullptr, 0, nullptr, nullptr, 0, c->sk_ws, ks[p], (wt & 1) ? wt : 0};
            if ((size_t)ks[p] * SK_ROWS * N > c->sk_ws_floats) return fail(TRACE_ERR_STATE, "partial-row workspace too small");
            return gemm_checked(g, EPI_PARTIAL, s, "partial GEMM");
        }
        if (r.kind == SK_W4A16) LCHK(launch_skinny_w4(X, K, P[p].w4c, P[p].w4e, B, N, K, c->sk_ws, c->sk_ws_floats, s));
        else if (r.kind == SK_W8A16) LCHK(launch_skinny_w8(X, K, P[p].w8d, P[p].sw, B, N, K, c->sk_ws, c->sk_ws_floats, s));
        else if (!f8) LCHK(launch_skinny_gemm(X, K, P[p].wd, K, nullptr, N, nullptr, 0, B, N, K, EPI_PARTIAL, 1, SKWS(c), s));
        else if (X == c->dH) LCHK(launch_skinny_fp8(c->dH8, K, c->dsh, P[p].w8d, P[p].sw, B, N, K, c->sk_ws, c->sk_ws_floats, s));
        else {
            LCHK(launch_quant_rows_fp8(X, K, c->dA8, K, c->dsa, B, K, s));
            LCHK(launch_skinny_fp8(c->dA8, K, c->dsa, P[p].w8d, P[p].sw, B, N, K, c->sk_ws, c->sk_ws_floats, s));
        }
        return TRACE_OK;
    };
    LCHK(launch_rmsnorm(c->dX, H, c->dH, H, c->llm[0].rms1, B, H, c->c.rms_eps, s));
    if (f8) LCHK(launch_quant_rows_fp8(c->dH, H, c->dH8, H, c->dsh, B, H, s));
    for (int l = 0; l < c->NL; ++l) {
        const LlmLayer& W = c->llm[l];
        P = layer_projs(W, H, I, QKV);
        // (fusing the RMSNorm into the GEMV itself was tried: re-scaling the same activations in every workgroup cost
        //  more than a row kernel — 65 us vs 52 + 6 us for the gate|up GEMV)
        TRY(proj(0, c->dH));
        if (r.qkv_finish) LCHK(qkv_finish_layer(c, l, r.ks_q, s));
        if (wide) {     // bracket bit 1, wide: the layer-0 decode attention, which streams the batch's whole KV cache of that layer
            StepBracket br(c, l, 3, s);
            if (br.e1) c->kbytes_sum += attn_kv_bytes(c);
            LCHK(attn_decode_layer(c, l, r, c->sk_ws, s));
        } else LCHK(attn_decode_layer(c, l, r, c->sk_ws, s));
        TRY(proj(1, c->dO));
        LCHK(launch_add_rmsnorm(c->sk_ws, r.ks_o, c->dX, H, c->dX, H, W.rms2, c->dH, H, B, H, c->c.rms_eps, s, f8 ? c->dH8 : nullptr, f8 ? c->dsh : nullptr));
        if (wide) {     // gate|up with the SwiGLU epilogue straight to bf16: no partial rows, no combine kernel
            GemmArgs gu{c->dH, H, (wt & 1) ? P[2].wd : P[2].w, H, c->dACT, I, nullptr, nullptr, 0, B, 2 * I, H, (wt & 1) ? nullptr : g_gemm_trace, 0, nullptr, nullptr, 0, nullptr, 0, (wt & 1) ? wt : 0};
            TRY(gemm_checked(gu, EPI_SWIGLU, s, "gate|up GEMM"));
        } else {
            {   // bracket bit 1, GEMV: the layer-0 gate|up GEMV (fp8: the bracket spans what the projection launches)
                StepBracket br(c, l, 1, s);
                TRY(proj(2, c->dH));
            }
            // (SwiGLU inside the gate|up GEMV at batch <= 16 — one K chunk, no combine kernel — measured 3.73 vs 3.5 ms per batch-1 step: its 224
            //  workgroups leave 32 CUs without a weight stream)
            LCHK(launch_swiglu_combine(c->sk_ws, r.ks_g, 2 * I, c->dACT, I, B, s));
        }
        TRY(proj(3, c->dACT));
        const bf16_t* nw = l + 1 < c->NL ? c->llm[l + 1].rms1 : c->final_norm;
        LCHK(launch_add_rmsnorm(c->sk_ws, r.ks_d, c->dX, H, c->dX, H, nw, c->dH, H, B, H, c->c.rms_eps, s, f8 ? c->dH8 : nullptr, f8 ? c->dsh : nullptr));
    }
    return head_and_select(c, c->dH, 1, logits_out, s);
}

// one decode step for the current batch: consumes dX (embedding of the last token), leaves the next one in dX
static int decode_step(trace_ctx* c, float* logits_out, hipStream_t s) {
    DecodeRoute r = decode_route(c->B, c->w4 ? 3 : c->fp8 ? 1 + c->fp8_wonly : 0, c->H, c->I, c->QKV, g_tune);    // (fp8 contexts: at most 64 rows, checked at begin)
    if (c->kv8) r.qkv_finish = true;                 // the e4m3 KV cache always appends with a launch of its own (qkv_finish_kv8), in every step body
    return r.step == 2 ? decode_step_fused(c, r, logits_out, s) : decode_step_rows(c, r, logits_out, s);
}

// The batch the NEXT trace_decode_begin starts holds the same K / V rows at positions below `rows` in every slot, and `slot` is one that holds them: the
// decode attention then reads those positions from that slot alone (whole 32-position blocks: rows is floored to a multiple of 32; below 32, or
// slot < 0, = off).  Consumed by that begin; a begin without a request before it decodes unshared.
extern "C" int trace_decode_set_shared_prefix(trace_ctx* c, int slot, int rows) {
    if (!c || !c->finalized) return fail(TRACE_ERR_STATE, "context not finalized");
    c->sh_want_slot = -1; c->sh_want_rows = 0;
    if (slot < 0 || rows < 32) return TRACE_OK;
    if (slot >= c->max_B || rows > c->max_ctx) return fail(TRACE_ERR_ARG, "shared slot / rows out of range");
    if (c->kv8) return fail(TRACE_ERR_STATE, "the shared prefix needs the 16-bit KV cache");
    c->sh_want_slot = slot; c->sh_want_rows = rows & ~31;
    return TRACE_OK;
}

static const char* row_params_convert(const trace_row_params& r, int cap, SampleParams& sp, LogitsParams& lp, int32_t& mx);
static const char* row_forced_bad(const trace_ctx* c, const int32_t* forced, int n, int max_new, const LogitsParams* lp, const int32_t* mx);
static bool logits_armed(const LogitsParams& p) { return p.penalty != 1.f || p.ngram != 0 || p.min_new != 0; }
static bool constraint_bans(const ConstrainTable& t) { return t.n_bad || t.n_suppress || t.n_begin; }

static int decode_cap(const trace_ctx* c) { return c->fp8 || c->w4 ? SKINNY_ROWS : SK_ROWS; }    // sequences that decode together on the context's kind of weights

// What trace_decode_begin and trace_decode_admit(_ex) share, in two halves with the entry point's own checks and state between them.
// seat_check: n prefilled sequences may take rows of the batch — slot in range and prefilled, no slot twice, head 0..2, the per-row params (rows at `stride`
// bytes; null: a batch without them) converted, prefill + max_new <= max_ctx, forced ids against the rows' processors.  who / who_rows prefix the messages.
struct Seated { int32_t pos[SK_ROWS]; std::vector<SampleParams> sp; std::vector<LogitsParams> lp; std::vector<int32_t> mx; bool procs = false; };
static int seat_check(trace_ctx* c, const std::string& who, const std::string& who_rows, int n, const int32_t* slots, const int32_t* heads, const int32_t* forced,
                      const trace_row_params* rows, size_t stride, int max_new, Seated& q) {
    q.sp.resize(rows ? n : 0); q.lp.resize(rows ? n : 0); q.mx.resize(rows ? n : 0);
    for (int i = 0; i < n; ++i) {
        if (slots[i] < 0 || slots[i] >= c->max_B || c->slot_len[slots[i]] <= 0) return fail(TRACE_ERR_STATE, who + "slot not prefilled");
        for (int j = 0; j < i; ++j) if (slots[j] == slots[i]) return fail(TRACE_ERR_ARG, who + "duplicate slot");
        if (heads[i] < 0 || heads[i] > 2) return fail(TRACE_ERR_ARG, who + "head must be 0, 1 or 2");
        q.pos[i] = c->slot_len[slots[i]];
        if (rows) {
            const trace_row_params* r = reinterpret_cast<const trace_row_params*>(reinterpret_cast<const char*>(rows) + (size_t)i * stride);   // (the caller's stride)
            if (r->size != rows[0].size) return fail(TRACE_ERR_ARG, who_rows + "every trace_row_params must carry the same size");
            if (const char* e = row_params_convert(*r, max_new, q.sp[i], q.lp[i], q.mx[i])) return fail(TRACE_ERR_ARG, who_rows + "row " + std::to_string(i) + ": " + e);
            q.procs = q.procs || logits_armed(q.lp[i]);       // a row brings armed logits processors
        }
        if (q.pos[i] + (rows ? q.mx[i] : max_new) > c->max_ctx) return fail(TRACE_ERR_ARG, who + "prefill + max_new_tokens exceeds max_ctx");
    }
    if (const char* e = rows ? row_forced_bad(c, forced, n, max_new, q.lp.data(), q.mx.data()) : nullptr) return fail(TRACE_ERR_ARG, who_rows + e);
    return TRACE_OK;
}
// seat_write: the checked sequences take rows [r0, r0 + n) — every column of row_cols gets its seat value, the rows' last prefill hidden rows are gathered,
// the head and the selection of their step 0 run on those rows alone with no position advance, and then the host mirrors and pos_sum follow.
static int seat_write(trace_ctx* c, int r0, int n, const int32_t* slots, const int32_t* heads, const int32_t* row_ids, const int32_t* forced, int origin,
                      const Seated& q, float* logits_out, hipStream_t s) {
    int32_t zero[SK_ROWS] = {0}, org[SK_ROWS];
    for (int i = 0; i < n; ++i) org[i] = origin;
    // seat values in row_cols' order: host rows to copy, else the byte the ints are filled with (forced: -1 = not forced; logprobs: entries past a row's
    // length stay 0.0), else (x, fill < 0) nothing: the selection below writes it
    const struct { const void* rows; int fill; } v[N_COLS] = {{slots}, {q.pos}, {heads}, {zero}, {zero}, {row_ids}, {org}, {nullptr, 0}, {forced, 0xff}, {nullptr, 0},
                                                              {q.sp.data()}, {q.lp.data()}, {q.mx.data()}, {nullptr, -1}};
    const auto col = row_cols(c);
    for (int k = 0; k < N_COLS; ++k) {
        int32_t* dst = col[k].dev + (size_t)r0 * col[k].ints;
        const size_t bytes = (size_t)n * col[k].ints * 4;
        if (!col[k].on) continue;
        if (v[k].rows) HIPCHK(hipMemcpyAsync(dst, v[k].rows, bytes, hipMemcpyHostToDevice, s));
        else if (v[k].fill >= 0) HIPCHK(hipMemsetAsync(dst, v[k].fill, bytes, s));
    }
    bf16_t* h = c->dH + (size_t)r0 * c->H;
    for (int i = 0; i < n; ++i)
        HIPCHK(hipMemcpyAsync(h + (size_t)i * c->H, c->xlast + (size_t)slots[i] * c->H, (size_t)c->H * 2, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));     // the host arrays above, and the caller's, must outlive the async copies
    TRY(head_and_select(c, h, 0, logits_out, s, TailRows{r0, n}));
    for (int k = 0; k < N_COLS; ++k)
        if (col[k].on && col[k].host) memcpy(static_cast<char*>(col[k].host) + (size_t)r0 * col[k].ints * 4, v[k].rows, (size_t)n * col[k].ints * 4);
    for (int i = 0; i < n; ++i) c->pos_sum += q.pos[i];
    return TRACE_OK;
}

extern "C" int trace_decode_begin(trace_ctx* c, const int32_t* slots, int B, const int32_t* heads, int max_new, int eos,
                                  const int32_t* forced, float* logits_out, void* stream) {
    if (!c || !c->finalized) return fail(TRACE_ERR_STATE, "context not finalized");
    // the per-row request (trace_decode_set_row_params) is this call's alone: taken here, whatever the call then answers
    std::vector<trace_row_params> want_rows;
    want_rows.swap(c->want_rows);
    if (!slots || !heads || B < 1 || B > c->max_B || B > decode_cap(c)) return fail(TRACE_ERR_ARG, "bad batch (at most " + std::to_string(decode_cap(c)) + " sequences decode together)");
    if (max_new < 1 || max_new > c->c.max_new_tokens) return fail(TRACE_ERR_ARG, "max_new exceeds capacity");
    hipStream_t s = (hipStream_t)stream;
    // the shared-prefix request is this call's alone: taken here, whatever the call then answers (one sequence shares with nobody)
    const int sh_slot = c->sh_want_slot, sh_rows = B > 1 ? c->sh_want_rows : 0;
    c->sh_want_slot = -1; c->sh_want_rows = 0;
    if (sh_rows > 0 && c->slot_len[sh_slot] < sh_rows) return fail(TRACE_ERR_STATE, "the shared slot holds fewer rows than the shared prefix");
    const bool per_row = !want_rows.empty();
    if (per_row && c->host_mode) return fail(TRACE_ERR_STATE, "per-row params are not available in host-select mode");
    if (per_row && (int)want_rows.size() != B) return fail(TRACE_ERR_ARG, "trace_decode_set_row_params gave " + std::to_string(want_rows.size()) + " rows, the batch has " + std::to_string(B));
    Seated q;
    TRY(seat_check(c, "", "", B, slots, heads, forced, per_row ? want_rows.data() : nullptr, sizeof(trace_row_params), max_new, q));
    int32_t iota[SK_ROWS];
    for (int b = 0; b < B; ++b) {
        iota[b] = b;
        if (c->slot_len[slots[b]] < sh_rows) return fail(TRACE_ERR_ARG, "a sequence is shorter than the shared prefix");
    }
    if (!per_row && forced && (c->want.process || c->want.stop) && !c->host_mode)
        return fail(TRACE_ERR_ARG, "logits processors / constraints (trace_decode_set_logits_params, trace_decode_set_constraints) with forced ids: the "
                                   "history is the recorded ids, not the fed ones");
    c->B = 0; c->max_new = max_new; c->eos = eos;         // (no batch until the rows are seated)
    c->sh_slot = sh_rows > 0 ? sh_slot : -1; c->sh_rows = sh_rows;
    c->pos_sum = 0; c->admitted = 0; c->fed = 0; c->steps_done = 0;
    // host-select mode arms nothing: the host holds the logits and calls trace_op_logits_process / trace_op_sample / trace_op_token_logprob on them
    c->armed = c->host_mode ? TailMode{} : c->want;
    if (per_row) {      // the batch-wide sampling and logits params are ignored: every row brings its own; constraints and log-probabilities stay the batch's
        TailMode m;
        m.per_row = true; m.logprobs = c->want.logprobs; m.stop = c->ctab.n_stop != 0;
        m.process = constraint_bans(c->ctab) || q.procs;
        c->armed = m;
    }
    const int32_t zero = 0, prm[3] = {max_new, eos, c->host_mode};
    HIPCHK(hipMemcpyAsync(c->d_step, &zero, 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->d_params, prm, 12, hipMemcpyHostToDevice, s));
    if (c->armed.sample) HIPCHK(hipMemcpyAsync(c->d_sparams, &c->samp, sizeof(SampleParams), hipMemcpyHostToDevice, s));
    if (c->armed.process) HIPCHK(hipMemcpyAsync(c->d_lgparams, &c->lgp, sizeof(LogitsParams), hipMemcpyHostToDevice, s));
    if (c->armed.process || c->armed.stop || per_row)       // the whole table, or the header alone when it is empty (the processors' kernel reads its four counts; a per-row batch may arm them at an admission)
        HIPCHK(hipMemcpyAsync(c->d_ctab, &c->ctab, constraints_on(c->ctab) ? sizeof(ConstrainTable) : 4 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    TRY(seat_write(c, 0, B, slots, heads, iota, forced, 0, q, logits_out, s));
    c->B = B;
    return TRACE_OK;
}

extern "C" int trace_decode_steps(trace_ctx* c, int n, int use_graph, float* logits_out, void* stream) {
    if (!c || c->B < 1) return fail(TRACE_ERR_STATE, "trace_decode_begin not called");
    if (n < 0) return fail(TRACE_ERR_ARG, "bad n");
    if (logits_out && (n != 1 || use_graph)) return fail(TRACE_ERR_ARG, "logits_out needs n == 1 and eager mode");
    if (c->host_mode && (n != 1 || use_graph)) return fail(TRACE_ERR_ARG, "host-select mode runs one eager step at a time");
    // every step appends one KV row at pos[b]++; decode_begin checked pos + max_new <= max_ctx once, so the total is bounded here
    if (!c->admitted && !c->armed.per_row) {
        if (c->steps_done + n > c->max_new - 1)
            return fail(TRACE_ERR_STATE, "decode steps exceed max_new - 1 since trace_decode_begin (" + std::to_string(c->steps_done) + " taken, " +
                                         std::to_string(n) + " requested, max_new " + std::to_string(c->max_new) + ")");
    } else {
        // After an admission the bound is per row: row b has taken steps_done - h_step0[b] steps of its own, and the call is refused only when no row
        // has room for all n.  A row whose own max_new is reached inside the call goes on being stepped with the batch; select_next_kernel's guard on
        // `local` stops its recording and its pos[b] += 1.  From the step's code (decode_step_*: append the fed token's K / V at row pos[b] of the slot,
        // attend rows [0, pos[b]], then select, which advances pos[b]): the row began at pos0 without an advance (its step 0), its local steps
        // 1 .. max_new - 1 appended at pos0 .. pos0 + max_new - 2 and left pos[b] = pos0 + max_new - 1; every later step (local >= max_new) appends at
        // that same row pos0 + max_new - 1 and attends pos0 + max_new rows.  The admission (like trace_decode_begin) checked pos0 + max_new <= max_ctx,
        // so pos0 + max_new - 1 <= max_ctx - 1: inside the row's own slot and inside the RoPE tables, whatever the number of such steps.
        int most = 0;                                 // the most steps any row of the batch may still take
        // With per-row params the same holds with the row's own max_new in place of the batch's: pos[b] stops at pos0 + own - 1, and begin / admit checked pos0 + own <= max_ctx.
        for (int b = 0; b < c->B; ++b) most = std::max(most, (c->armed.per_row ? c->h_row_max[b] : c->max_new) - 1 - (c->steps_done - c->h_step0[b]));
        if (n > most)
            return fail(TRACE_ERR_STATE, "decode steps exceed max_new - 1 for every row of the batch (" + std::to_string(n) + " requested, at most " +
                                         std::to_string(most) + " left to any row, max_new " + std::to_string(c->max_new) + ")");
    }
    const int steps_before = c->steps_done;
    c->steps_done += n;
    hipStream_t s = (hipStream_t)stream;
    if (c->profile) hipEventRecord(c->ev0, s);
    if (!use_graph) {
        for (int i = 0; i < n; ++i) { c->step_in_call = steps_before + i; TRY(decode_step(c, logits_out, s)); }
    } else {
        trace_ctx::StepGraph* ways = c->graphs[c->armed.index()][c->B];     // (index() < TAIL_MODES by its construction)
        trace_ctx::StepGraph* way = nullptr;
        for (int w = 0; w < 2 && !way; ++w)
            if (ways[w].exec && ways[w].sh_slot == c->sh_slot && ways[w].sh_rows == c->sh_rows) way = &ways[w];
        if (!way) {
            way = !ways[0].exec ? &ways[0] : !ways[1].exec ? &ways[1] : &ways[c->graph_evict ^= 1];
            if (way->exec) { HIPCHK(hipStreamSynchronize(s)); hipGraphExecDestroy(way->exec); way->exec = nullptr; }
            way->sh_slot = c->sh_slot; way->sh_rows = c->sh_rows;
        }
        hipGraphExec_t* slot_g = &way->exec;
        if (!*slot_g) {
            hipGraph_t g = nullptr;
            HIPCHK(hipStreamSynchronize(s));
            HIPCHK(hipStreamBeginCapture(c->cap_stream, hipStreamCaptureModeThreadLocal));   // another thread may be launching the encode stage (generate_stream)
            const int rc = decode_step(c, nullptr, c->cap_stream);
            hipError_t e = hipStreamEndCapture(c->cap_stream, &g);
            if (rc != TRACE_OK) { if (g) hipGraphDestroy(g); return rc; }
            if (e != hipSuccess) return fail(TRACE_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
            e = hipGraphInstantiate(slot_g, g, nullptr, nullptr, 0);
            hipGraphDestroy(g);
            if (e != hipSuccess) { *slot_g = nullptr; return fail(TRACE_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e)); }
        }
        for (int i = 0; i < n; ++i) HIPCHK(hipGraphLaunch(*slot_g, s));
    }
    if (c->profile == 2 && c->kev_used > 0) {   // drain the eager-mode brackets
        hipStreamSynchronize(s);
        for (int i = 0; i + 1 < c->kev_used; i += 2) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, c->kev[i], c->kev[i + 1]) == hipSuccess) { c->ksum_ms += ms; c->ksamples += 1; }
        }
        c->kev_used = 0;
    }
    if (c->profile) {
        hipEventRecord(c->ev1, s);
        hipEventSynchronize(c->ev1);
        float ms = 0.f;
        hipEventElapsedTime(&ms, c->ev0, c->ev1);
        c->prof[0] = n > 0 ? ms / n : 0.f;
        c->prof[1] = (float)n;
        c->prof[2] = c->ksamples ? (float)(c->ksum_ms / c->ksamples) : 0.f;
        c->prof[3] = (float)c->ksamples;
        // algorithmic bytes of the bracketed launch, by WHICH launch took the bracket (bracket_kind — not by the batch size: the wide step starts at
        // decode.wide_min_rows rows, below SKINNY_ROWS): the gate|up weights (fp8: the bracket also spans the activation quantiser), or the layer-0
        // attention's KV rows averaged over the bracketed steps
        c->prof[4] = (float)(2.0 * c->I * c->H * (c->w4 ? 0.53125 : c->fp8 ? 1.0 : 2.0));
        if (c->bracket_kind == 3 && c->ksamples) c->prof[4] = (float)(c->kbytes_sum / c->ksamples);
        c->prof[8] = (float)c->bracket_kind;
    }
    return TRACE_OK;
}

// Shrink the running batch to the rows keep[0 .. n_keep): everything a step reads or writes per row moves with the row (retire.hip), the host copy
// of the batch follows, and the next trace_decode_steps runs (captures, the first time) the step of the new batch size.
extern "C" int trace_decode_retire(trace_ctx* c, const int32_t* keep, int n_keep, void* stream) {
    if (!c || c->B < 1) return fail(TRACE_ERR_STATE, "trace_decode_begin not called");
    if (c->host_mode) return fail(TRACE_ERR_STATE, "trace_decode_retire is not available in host-select mode");
    const int B = c->B;
    if (!keep || n_keep < 1 || n_keep > B) return fail(TRACE_ERR_ARG, "n_keep must lie in [1, " + std::to_string(B) + "] (the rows of the running batch)");
    for (int i = 0; i < n_keep; ++i) {
        if (keep[i] < 0 || keep[i] >= B) return fail(TRACE_ERR_ARG, "keep[" + std::to_string(i) + "] = " + std::to_string(keep[i]) + " is outside [0, " + std::to_string(B) + ")");
        if (i && keep[i] <= keep[i - 1]) return fail(TRACE_ERR_ARG, "the keep list must be strictly increasing");
    }
    if (n_keep == B) return TRACE_OK;                // every row, in order: nothing moves, nothing is launched
    hipStream_t s = (hipStream_t)stream;
    const size_t row_ints = retire_row_ints(c->c.max_new_tokens, c->H);
    if (!c->d_retire) TRY(dalloc(c, &c->d_retire, SK_ROWS + SK_ROWS * row_ints));
    const auto col = row_cols(c);
    auto dev = [&](int k) { return col[k].on ? col[k].dev : nullptr; };      // (null where the armed mode has no such column)
    RetireArgs a{};
    for (int k = 0; k < RETIRE_SMALL; ++k) a.small[k] = dev(k);
    for (int k = 0; k < 3; ++k) { a.wide[k] = dev(RETIRE_SMALL + k); a.rowp[k] = dev(RETIRE_SMALL + 3 + k); }
    a.x = c->dX; a.H = c->H; a.max_new = c->max_new;
    HIPCHK(hipMemcpyAsync(c->d_retire, keep, (size_t)n_keep * 4, hipMemcpyHostToDevice, s));
    LCHK(launch_retire(a, c->d_retire, n_keep, B, c->d_retire + SK_ROWS, s));
    HIPCHK(hipStreamSynchronize(s));                 // the caller's keep list must outlive the async copy
    for (const RowCol& k : col)                      // the host mirrors follow (keep[i] >= i: read before overwritten)
        for (int i = 0; k.on && k.host && i < n_keep; ++i)
            memmove(static_cast<char*>(k.host) + (size_t)i * k.ints * 4, static_cast<char*>(k.host) + (size_t)keep[i] * k.ints * 4, (size_t)k.ints * 4);
    c->pos_sum = 0;
    for (int i = 0; i < n_keep; ++i) c->pos_sum += c->h_pos0[i];
    c->B = n_keep;
    if (n_keep == 1) { c->sh_slot = -1; c->sh_rows = 0; }      // one sequence shares with nobody (as at trace_decode_begin): its own slot holds the same rows
    return TRACE_OK;
}

// Append n prefilled sequences behind the B rows of the running batch (retire first, then admit: rows never land in holes).  What trace_decode_begin
// does for a batch is done for rows [B, B + n) alone; then the head and the selection of their own step 0 run on those rows only, no position advance.
// The counter, and why no launch can see it half-advanced: the selection's check-in (select.h) lets the last of a launch's workgroups advance the
// counter it was given.  The admission's launches get the spare pair d_step[2..3] (TailRows), zeroed by a stream-ordered copy before them, and a null
// origin: their `local` is 0, they check in n times to the spare pair, and nothing of theirs reads or writes d_step[0..1] or a row in front of B.  The
// shared counter therefore still holds what the last step of the batch left, steps_done + 1 (trace_decode_begin's selection took it from 0 to 1, every
// step adds 1), and the origin of the new rows is written by the host from that number, steps_done: the next common step reads counter steps_done + 1,
// their local step 1.  Everything is queued on the caller's stream, in order, between two steps; the next step's graph or launches see B + n rows
// whose check-in count is B + n, so its last workgroup, and no earlier one, advances the shared counter.
// rows: one trace_row_params per admitted row, for a batch begun with them (and only for such a batch) — written at [B, B + n) of the per-row arrays before
// the rows' token 0 is selected.
extern "C" int trace_decode_admit_ex(trace_ctx* c, const int32_t* slots, int n, const int32_t* heads, const int32_t* row_ids, const int32_t* forced,
                                     const trace_row_params* rows, void* stream) {
    if (!c || c->B < 1) return fail(TRACE_ERR_STATE, "trace_decode_admit: no decode batch is running (trace_decode_begin not called)");
    if (c->host_mode) return fail(TRACE_ERR_STATE, "trace_decode_admit is not available in host-select mode");
    if (c->sh_rows > 0) return fail(TRACE_ERR_STATE, "trace_decode_admit: the running batch attends a shared prefix; admitted rows would have to hold the same rows");
    if (!slots || !heads || !row_ids || n < 1) return fail(TRACE_ERR_ARG, "trace_decode_admit: bad slots / heads / row_ids / n");
    const bool per_row = c->armed.per_row;
    if (per_row && !rows) return fail(TRACE_ERR_STATE, "trace_decode_admit: the running batch was begun with per-row params; admit into it through trace_decode_admit_ex with rows");
    if (!per_row && rows) return fail(TRACE_ERR_STATE, "trace_decode_admit_ex: the running batch was begun without per-row params (trace_decode_set_row_params)");
    const int B = c->B, cap = std::min(c->max_B, decode_cap(c));
    if (n > cap - B) return fail(TRACE_ERR_ARG, "trace_decode_admit: " + std::to_string(B) + " running + " + std::to_string(n) + " admitted rows exceed the cap (at most " + std::to_string(cap) + " sequences decode together)");
    if (per_row && rows[0].size < (int32_t)sizeof(trace_row_params)) return fail(TRACE_ERR_ARG, "trace_row_params::size is smaller than this library's struct");
    Seated q;
    TRY(seat_check(c, "trace_decode_admit: ", "trace_decode_admit_ex: ", n, slots, heads, forced, rows, per_row ? (size_t)rows[0].size : 0, c->max_new, q));
    for (int i = 0; i < n; ++i) {
        for (int b = 0; b < B; ++b) if (c->h_slots[b] == slots[i]) return fail(TRACE_ERR_ARG, "trace_decode_admit: slot " + std::to_string(slots[i]) + " is already in the running batch");
        if (row_ids[i] < 0) return fail(TRACE_ERR_ARG, "trace_decode_admit: row_ids must not be negative");
    }
    if (!per_row && forced && (c->armed.process || c->armed.stop))
        return fail(TRACE_ERR_ARG, "trace_decode_admit: forced ids with logits processors / constraints armed: the history is the recorded ids, not the fed ones");
    hipStream_t s = (hipStream_t)stream;
    const int32_t zero[2] = {0, 0};
    if (q.procs) c->armed.process = true;            // from here on logits_process runs for the batch (a tail of its own graph place)
    HIPCHK(hipMemcpyAsync(c->d_step + 2, zero, 8, hipMemcpyHostToDevice, s));          // the spare counter pair of the admission's own selection
    TRY(seat_write(c, B, n, slots, heads, row_ids, forced, c->steps_done, q, nullptr, s));
    c->B = B + n; c->admitted += n;
    return TRACE_OK;
}

extern "C" int trace_decode_admit(trace_ctx* c, const int32_t* slots, int n, const int32_t* heads, const int32_t* row_ids, const int32_t* forced,
                                  void* stream) {
    return trace_decode_admit_ex(c, slots, n, heads, row_ids, forced, nullptr, stream);
}

extern "C" int trace_debug_step_graphs(trace_ctx* c, int32_t* sizes, int cap) {
    if (!c) return 0;
    int n = 0;
    for (int B = 1; B <= SK_ROWS; ++B) {
        bool any = false;
        for (int m = 0; m < TAIL_MODES && !any; ++m) any = c->graphs[m][B][0].exec || c->graphs[m][B][1].exec;
        if (any) { if (sizes && n < cap) sizes[n] = B; ++n; }
    }
    return n;
}

// Debugging aid: one column of row_cols for rows [0, B) of the running batch, as ints, into out[0 .. cap) (HOST); synchronous.  Returns the column's ints
// a row, or 0 (nothing written) for a column the armed mode does not have.  trace_debug_decode_column(ctx, i) names column i, NULL past the end.
extern "C" int trace_debug_decode_rows(trace_ctx* c, int column, int32_t* out, int cap) {
    if (!c || c->B < 1) return fail(TRACE_ERR_STATE, "trace_decode_begin not called");
    if (column < 0 || column >= N_COLS || !out) return fail(TRACE_ERR_ARG, "trace_debug_decode_rows: bad column / out");
    const RowCol k = row_cols(c)[column];
    if (!k.on) return 0;
    if ((size_t)cap < (size_t)c->B * k.ints) return fail(TRACE_ERR_ARG, "trace_debug_decode_rows: cap is below B x " + std::to_string(k.ints) + " ints");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, k.dev, (size_t)c->B * k.ints * 4, hipMemcpyDeviceToHost));
    return k.ints;
}
extern "C" const char* trace_debug_decode_column(trace_ctx* c, int i) { return c && i >= 0 && i < N_COLS ? row_cols(c)[i].name : nullptr; }

extern "C" int trace_decode_read(trace_ctx* c, int32_t* out_ids, int32_t* out_len, int32_t* heads, void* stream) {
    if (!c || c->B < 1) return fail(TRACE_ERR_STATE, "trace_decode_begin not called");
    hipStream_t s = (hipStream_t)stream;
    if (out_ids) HIPCHK(hipMemcpyAsync(out_ids, c->d_out_ids, (size_t)c->B * c->max_new * 4, hipMemcpyDeviceToHost, s));
    if (out_len) HIPCHK(hipMemcpyAsync(out_len, c->d_out_len, c->B * 4, hipMemcpyDeviceToHost, s));
    if (heads) HIPCHK(hipMemcpyAsync(heads, c->d_heads, c->B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return TRACE_OK;
}

// the device sampler's domain (sample.h): T > 0 finite, 0 < p <= 1, k in [1, 1024], or k = 0 with p = 1
static const char* sampling_bad(float T, int k, float p) {
    if (!(T > 0.f) || !std::isfinite(T)) return "temperature must be a finite number > 0";
    if (!(p > 0.f && p <= 1.f)) return "top_p must lie in (0, 1]";
    if (k < 0 || k > SAMPLE_MAX_K) return "top_k must lie in [0, 1024] on the device";
    if (k == 0 && p < 1.f) return "top_k = 0 (off) with top_p < 1 is outside the device sampler (sort of the whole head)";
    return nullptr;
}
// the four warpers behind top_p (trace_sampling): HF's domains, off values accepted, and top_k in [1, 1024] once one of them is armed
static const char* warpers_bad(const trace_sampling& t) {
    if (!(t.min_p >= 0.f && t.min_p <= 1.f)) return "min_p must lie in [0, 1]";
    if (!(t.typical_p > 0.f && t.typical_p <= 1.f)) return "typical_p must lie in (0, 1] (1 = off)";
    if (!(t.epsilon_cutoff >= 0.f && t.epsilon_cutoff < 1.f)) return "epsilon_cutoff must lie in [0, 1) (0 = off)";
    if (!(t.eta_cutoff >= 0.f && t.eta_cutoff < 1.f)) return "eta_cutoff must lie in [0, 1) (0 = off)";
    const bool armed = t.min_p > 0.f || t.typical_p < 1.f || t.epsilon_cutoff > 0.f || t.eta_cutoff > 0.f;
    if (armed && t.top_k < 1)
        return "top_k = 0 (off) with min_p / typical_p / epsilon_cutoff / eta_cutoff armed is outside the device sampler (sort of the whole head)";
    return nullptr;
}
// a trace_sampling is checked in this order everywhere: the struct itself (null, size), then - behind the greedy shortcut of the decode entry - the domain
static const char* sampling_struct_bad(const trace_sampling* t) {
    if (!t) return "null trace_sampling";
    if (t->size < (int32_t)sizeof(trace_sampling)) return "trace_sampling::size is smaller than this library's struct";
    return nullptr;
}
static const char* sampling_domain_bad(const trace_sampling& t) {
    if (const char* e = sampling_bad(t.temperature, t.top_k, t.top_p)) return e;
    return warpers_bad(t);
}
static SampleParams make_sampling(float T, int k, float p, uint64_t seed) {
    SampleParams sp{};
    sp.temperature = T; sp.top_k = k; sp.top_p = p; sp.seed_lo = (uint32_t)seed; sp.seed_hi = (uint32_t)(seed >> 32);
    sp.min_p = 0.f; sp.typical_p = 1.f; sp.epsilon = 0.f; sp.eta = 0.f; sp.sqrt_eta = 0.f;                    // the four off
    return sp;
}
static SampleParams make_sampling(const trace_sampling& t) {
    SampleParams sp = make_sampling(t.temperature, t.top_k, t.top_p, t.seed);
    sp.min_p = t.min_p; sp.typical_p = t.typical_p; sp.epsilon = t.epsilon_cutoff; sp.eta = t.eta_cutoff; sp.sqrt_eta = sqrtf(t.eta_cutoff);
    return sp;
}

// The requested tail mode becomes m, once the buffers it needs exist (allocated on first use): the raw rows for any request, the processed rows,
// the log-probabilities, the constraint table.  A context that never requests anything allocates none of them.  m.process and m.stop follow from the
// logits params and the constraint table the context holds: process = any param or any ban rule armed, stop = any stop sequence.
static int set_want(trace_ctx* c, TailMode m) {
    m.process = c->lgp.penalty != 1.f || c->lgp.ngram != 0 || c->lgp.min_new != 0 || c->ctab.n_bad || c->ctab.n_suppress || c->ctab.n_begin;
    m.stop = c->ctab.n_stop != 0;
    if ((m.process || m.stop) && !c->d_ctab) {
        TRY(dalloc(c, &c->d_ctab, 1));
        HIPCHK(hipMemset(c->d_ctab, 0, sizeof(ConstrainTable)));
    }
    if (m.index() && !c->d_slog) TRY(dalloc(c, &c->d_slog, (size_t)SK_ROWS * c->NV));
    if (m.process && !c->d_plog) TRY(dalloc(c, &c->d_plog, (size_t)SK_ROWS * c->NV));
    if (m.logprobs && !c->d_logprobs) TRY(dalloc(c, &c->d_logprobs, (size_t)SK_ROWS * c->c.max_new_tokens));
    c->want = m;
    return TRACE_OK;
}

extern "C" int trace_decode_set_sampling(trace_ctx* c, float temperature, int top_k, float top_p, uint64_t seed) {
    if (!c || !c->finalized) return fail(TRACE_ERR_STATE, "context not finalized");
    if (std::isnan(temperature)) return fail(TRACE_ERR_ARG, "temperature is NaN");
    TailMode m = c->want;
    m.sample = temperature > 0.f;                                          // <= 0: greedy
    if (!m.sample) return set_want(c, m);
    if (const char* e = sampling_bad(temperature, top_k, top_p)) return fail(TRACE_ERR_ARG, e);
    c->samp = make_sampling(temperature, top_k, top_p, seed);
    return set_want(c, m);
}

extern "C" int trace_decode_set_sampling_ex(trace_ctx* c, const trace_sampling* t) {
    if (!c || !c->finalized) return fail(TRACE_ERR_STATE, "context not finalized");
    if (const char* e = sampling_struct_bad(t)) return fail(TRACE_ERR_ARG, e);
    if (t->temperature <= 0.f) return trace_decode_set_sampling(c, 0.f, 0, 1.f, 0);                      // greedy: the other fields are not read
    if (const char* e = sampling_domain_bad(*t)) return fail(TRACE_ERR_ARG, e);
    TailMode m = c->want;
    m.sample = true;
    c->samp = make_sampling(*t);
    return set_want(c, m);
}

extern "C" int trace_decode_set_logprobs(trace_ctx* c, int on) {
    if (!c || !c->finalized) return fail(TRACE_ERR_STATE, "context not finalized");
    TailMode m = c->want;
    m.logprobs = on != 0;
    return set_want(c, m);
}

static const char* logits_params_bad(float p, int n, int m) {
    if (!(p > 0.f) || !std::isfinite(p)) return "repetition_penalty must be a finite number > 0";
    if (n < 0 || n > LOGITS_MAX_NGRAM) return "no_repeat_ngram_size must lie in [0, 64]";
    if (m < 0) return "min_new_tokens must not be negative";
    return nullptr;
}

extern "C" int trace_decode_set_logits_params(trace_ctx* c, float repetition_penalty, int no_repeat_ngram_size, int min_new_tokens) {
    if (!c || !c->finalized) return fail(TRACE_ERR_STATE, "context not finalized");
    if (const char* m = logits_params_bad(repetition_penalty, no_repeat_ngram_size, min_new_tokens)) return fail(TRACE_ERR_ARG, m);
    c->lgp = LogitsParams{repetition_penalty, no_repeat_ngram_size, min_new_tokens};
    return set_want(c, c->want);
}

// ---- per-row generation parameters ----
// one trace_row_params -> the device structs of its row; a message, or null.  cap: the largest max_new the row may ask for
static const char* row_params_convert(const trace_row_params& r, int cap, SampleParams& sp, LogitsParams& lp, int32_t& mx) {
    if (r.size < (int32_t)sizeof(trace_row_params)) return "trace_row_params::size is smaller than this library's struct";
    if (std::isnan(r.sampling.temperature)) return "temperature is NaN";
    sp = SampleParams{};                                                   // temperature 0: the row is greedy, the rest of `sampling` is not read
    if (r.sampling.temperature > 0.f) {
        if (const char* e = sampling_struct_bad(&r.sampling)) return e;
        if (const char* e = sampling_domain_bad(r.sampling)) return e;
        sp = make_sampling(r.sampling);
    }
    if (const char* e = logits_params_bad(r.repetition_penalty, r.no_repeat_ngram_size, r.min_new_tokens)) return e;
    lp = LogitsParams{r.repetition_penalty, r.no_repeat_ngram_size, r.min_new_tokens};
    if (r.max_new < 1 || r.max_new > cap) return "max_new of a row must lie in [1, the max_new given to trace_decode_begin]";
    mx = r.max_new;
    return nullptr;
}
// forced ids [n][max_new] against the rows' processors: refused for a row whose processors are armed and that is fed an id within its own max_new, and
// for any row once the constraints are armed (the history is the recorded ids, not the fed ones)
static const char* row_forced_bad(const trace_ctx* c, const int32_t* forced, int n, int max_new, const LogitsParams* lp, const int32_t* mx) {
    if (!forced) return nullptr;
    if (constraint_bans(c->ctab) || c->ctab.n_stop) return "forced ids with constraints armed: the history is the recorded ids, not the fed ones";
    for (int b = 0; b < n; ++b) {
        if (!logits_armed(lp[b])) continue;
        for (int i = 0; i < mx[b]; ++i)
            if (forced[(size_t)b * max_new + i] >= 0) return "forced ids on a row whose logits processors are armed: the history is the recorded ids, not the fed ones";
    }
    return nullptr;
}

extern "C" int trace_decode_set_row_params(trace_ctx* c, const trace_row_params* rows, int n) {
    if (!c || !c->finalized) return fail(TRACE_ERR_STATE, "context not finalized");
    c->want_rows.clear();
    if (!rows || n == 0) return TRACE_OK;
    if (c->host_mode) return fail(TRACE_ERR_STATE, "per-row params are not available in host-select mode");
    if (n < 0 || n > SK_ROWS) return fail(TRACE_ERR_ARG, "trace_decode_set_row_params: n must lie in [0, 256]");
    if (rows[0].size < (int32_t)sizeof(trace_row_params)) return fail(TRACE_ERR_ARG, "trace_row_params::size is smaller than this library's struct");
    std::vector<trace_row_params> take(n);
    for (int i = 0; i < n; ++i) {
        const trace_row_params* r = reinterpret_cast<const trace_row_params*>(reinterpret_cast<const char*>(rows) + (size_t)i * rows[0].size);   // (the caller's stride)
        if (r->size != rows[0].size) return fail(TRACE_ERR_ARG, "trace_decode_set_row_params: every trace_row_params must carry the same size");
        SampleParams sp; LogitsParams lp; int32_t mx;
        if (const char* e = row_params_convert(*r, c->c.max_new_tokens, sp, lp, mx)) return fail(TRACE_ERR_ARG, "trace_decode_set_row_params: row " + std::to_string(i) + ": " + e);
        take[i] = *r;
    }
    // what the tail of such a batch may read: the raw rows, the processed rows (a row's processors may arm them at an admission), the constraint table
    if (!c->d_ctab) {
        TRY(dalloc(c, &c->d_ctab, 1));
        HIPCHK(hipMemset(c->d_ctab, 0, sizeof(ConstrainTable)));
    }
    if (!c->d_slog) TRY(dalloc(c, &c->d_slog, (size_t)SK_ROWS * c->NV));
    if (!c->d_plog) TRY(dalloc(c, &c->d_plog, (size_t)SK_ROWS * c->NV));
    c->want_rows.swap(take);
    return TRACE_OK;
}

// trace_constraints -> the table, bounded and checked: a message, or null.  NV > 0: every id must lie in [0, NV).
static const char* constraints_table(const trace_constraints* k, int NV, ConstrainTable& t) {
    memset(&t, 0, sizeof(t));
    if (!k) return nullptr;
    if (k->size < (int32_t)sizeof(trace_constraints)) return "trace_constraints.size is smaller than the struct";
    if (k->n_stop < 0 || k->n_stop > CONSTRAIN_MAX_SEQS) return "at most 64 stop sequences";
    if (k->n_bad_words < 0 || k->n_bad_words > CONSTRAIN_MAX_SEQS) return "at most 64 bad-word sequences";
    if (k->n_suppress < 0 || k->n_suppress > CONSTRAIN_MAX_SUPPRESS || k->n_begin_suppress < 0 || k->n_begin_suppress > CONSTRAIN_MAX_SUPPRESS)
        return "at most 1024 ids in each suppress list";
    auto id_ok = [NV](int32_t v) { return v >= 0 && (NV <= 0 || v < NV); };
    auto csr = [&](int n, const int32_t* off, const int32_t* ids, int32_t* toff, int32_t* tids) -> const char* {
        if (n == 0) return nullptr;
        if (!off || !ids) return "null offsets / ids of a sequence list";
        if (off[0] != 0) return "sequence offsets must start at 0";
        for (int i = 0; i < n; ++i) {
            const int len = off[i + 1] - off[i];
            if (len < 1) return "an empty sequence (or offsets that do not ascend)";
            if (len > CONSTRAIN_MAX_SEQ_LEN) return "at most 32 ids per sequence";
        }
        for (int i = 0; i <= n; ++i) toff[i] = off[i];
        for (int j = 0; j < off[n]; ++j) {
            if (!id_ok(ids[j])) return "a sequence id outside the vocabulary";
            tids[j] = ids[j];
        }
        return nullptr;
    };
    auto flat = [&](int n, const int32_t* ids, int32_t* tids) -> const char* {
        if (n == 0) return nullptr;
        if (!ids) return "null suppress list";
        for (int j = 0; j < n; ++j) {
            if (!id_ok(ids[j])) return "a suppressed id outside the vocabulary";
            tids[j] = ids[j];
        }
        return nullptr;
    };
    if (const char* m = csr(k->n_stop, k->stop_offsets, k->stop_ids, t.stop_off, t.stop_ids)) return m;
    if (const char* m = csr(k->n_bad_words, k->bad_word_offsets, k->bad_word_ids, t.bad_off, t.bad_ids)) return m;
    if (const char* m = flat(k->n_suppress, k->suppress_ids, t.suppress)) return m;
    if (const char* m = flat(k->n_begin_suppress, k->begin_suppress_ids, t.begin)) return m;
    t.n_stop = k->n_stop; t.n_bad = k->n_bad_words; t.n_suppress = k->n_suppress; t.n_begin = k->n_begin_suppress;
    return nullptr;
}

extern "C" int trace_decode_set_constraints(trace_ctx* c, const trace_constraints* k) {
    if (!c || !c->finalized) return fail(TRACE_ERR_STATE, "context not finalized");
    ConstrainTable t;
    if (const char* m = constraints_table(k, c->NV, t)) return fail(TRACE_ERR_ARG, m);
    c->ctab = t;
    return set_want(c, c->want);
}

// the loose-row ops' device copy of a table: one buffer per device for the life of the process, rewritten by every call on the call's stream (the
// stream is drained before the call returns: the host copy is a local, and a later call may rewrite the buffer)
static int loose_table(const ConstrainTable& t, hipStream_t s, ConstrainTable** out) {
    static ConstrainTable* d_tab[16] = {nullptr};
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (dev < 0 || dev >= 16) return fail(TRACE_ERR_ARG, "device index out of range");
    if (!d_tab[dev]) HIPCHK(hipMalloc((void**)&d_tab[dev], sizeof(ConstrainTable)));
    HIPCHK(hipMemcpyAsync(d_tab[dev], &t, sizeof(ConstrainTable), hipMemcpyHostToDevice, s));
    *out = d_tab[dev];
    return TRACE_OK;
}

extern "C" int trace_op_logits_process_ex(const float* logits, int ld, int B, const int32_t* heads, int V, int Tv, int Sv, const int32_t* hist, int ld_hist,
                                          const int32_t* hist_len, const int32_t* steps, int eos, float repetition_penalty, int no_repeat_ngram_size,
                                          int min_new_tokens, const trace_constraints* constraints, float* out, void* stream) {
    if (!logits || !heads || !hist || !hist_len || !steps || !out) return fail(TRACE_ERR_ARG, "null pointer");
    if (out == logits) return fail(TRACE_ERR_ARG, "out may not alias logits");
    if (const char* m = logits_params_bad(repetition_penalty, no_repeat_ngram_size, min_new_tokens)) return fail(TRACE_ERR_ARG, m);
    if (V < 1 || Tv < 1 || Sv < 1) return fail(TRACE_ERR_ARG, "bad head widths");
    ConstrainTable t;
    if (const char* m = constraints_table(constraints, V + 1 + Tv + Sv, t)) return fail(TRACE_ERR_ARG, m);
    hipStream_t s = (hipStream_t)stream;
    ConstrainTable* dt = nullptr;
    TRY(loose_table(t, s, &dt));
    const int rc = launch_logits_process(logits, ld, B, heads, V, Tv, Sv, hist, ld_hist, hist_len, steps, eos,
                                         LogitsParams{repetition_penalty, no_repeat_ngram_size, min_new_tokens}, out, ld, s, dt);
    HIPCHK(hipStreamSynchronize(s));
    if (rc != TRACE_OK) return fail(rc, "logits_process launch failed (B, ld, ld_hist or head widths out of range)");
    return TRACE_OK;
}

extern "C" int trace_op_stop_match(const int32_t* hist, int ld_hist, const int32_t* hist_len, int B, const trace_constraints* constraints,
                                   int32_t* fired_out, void* stream) {
    if (!hist || !hist_len || !fired_out) return fail(TRACE_ERR_ARG, "null pointer");
    if (B < 1 || B > 65535 || ld_hist < 0) return fail(TRACE_ERR_ARG, "bad B / ld_hist");
    ConstrainTable t;
    if (const char* m = constraints_table(constraints, 0, t)) return fail(TRACE_ERR_ARG, m);
    hipStream_t s = (hipStream_t)stream;
    ConstrainTable* dt = nullptr;
    TRY(loose_table(t, s, &dt));
    const int rc = launch_stop_match(hist, ld_hist, hist_len, B, dt, fired_out, s);
    HIPCHK(hipStreamSynchronize(s));
    if (rc != TRACE_OK) return fail(rc, "stop_match launch failed");
    return TRACE_OK;
}

extern "C" int trace_op_logits_process(const float* logits, int ld, int B, const int32_t* heads, int V, int Tv, int Sv, const int32_t* hist, int ld_hist,
                                       const int32_t* hist_len, const int32_t* steps, int eos, float repetition_penalty, int no_repeat_ngram_size,
                                       int min_new_tokens, float* out, void* stream) {
    if (!logits || !heads || !hist || !hist_len || !steps || !out) return fail(TRACE_ERR_ARG, "null pointer");
    if (out == logits) return fail(TRACE_ERR_ARG, "out may not alias logits");
    if (const char* m = logits_params_bad(repetition_penalty, no_repeat_ngram_size, min_new_tokens)) return fail(TRACE_ERR_ARG, m);
    const int rc = launch_logits_process(logits, ld, B, heads, V, Tv, Sv, hist, ld_hist, hist_len, steps, eos,
                                         LogitsParams{repetition_penalty, no_repeat_ngram_size, min_new_tokens}, out, ld, (hipStream_t)stream);
    if (rc != TRACE_OK) return fail(rc, "logits_process launch failed (B, ld, ld_hist or head widths out of range)");
    return TRACE_OK;
}

extern "C" int trace_decode_read_logprobs(trace_ctx* c, float* out, void* stream) {
    if (!c || c->B < 1) return fail(TRACE_ERR_STATE, "trace_decode_begin not called");
    if (!c->armed.logprobs) return fail(TRACE_ERR_STATE, "the current batch was begun without log-probabilities (trace_decode_set_logprobs)");
    if (!out) return fail(TRACE_ERR_ARG, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(out, c->d_logprobs, (size_t)c->B * c->max_new * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return TRACE_OK;
}

extern "C" int trace_op_token_logprob(const float* logits, int ld, int B, const int32_t* heads, int V, int Tv, int Sv, const int32_t* ids, float* out,
                                      void* stream) {
    if (!logits || !heads || !ids || !out) return fail(TRACE_ERR_ARG, "null pointer");
    const int rc = launch_token_logprob(logits, ld, B, heads, V, Tv, Sv, ids, out, (hipStream_t)stream);
    if (rc != TRACE_OK) return fail(rc, "token_logprob launch failed (B, ld or head widths out of range)");
    return TRACE_OK;
}

// ---- scoring given tokens (score.hip) ----
extern "C" int trace_op_score_tile(void) { return SCORE_TILE; }
extern "C" int64_t trace_op_score_ws_bytes(int R, int V, int Tv, int Sv) {
    if (R < 1 || R > SCORE_MAX_ROWS || V < 1 || Tv < 1 || Sv < 1) return fail(TRACE_ERR_ARG, "bad R / head widths");
    return (int64_t)score_ws_floats(R, V) * 4;
}
extern "C" int trace_op_score_rows(const void* hidden, int ld, const void* W, int ldw, int K, int R, const int32_t* heads, const int32_t* ids, int V, int Tv,
                                   int Sv, void* ws, float* out, void* stream) {
    if (!hidden || !W || !heads || !ids || !ws || !out) return fail(TRACE_ERR_ARG, "null pointer");
    const int rc = launch_score_rows((const bf16_t*)hidden, ld, (const bf16_t*)W, ldw, K, R, heads, ids, V, Tv, Sv, (float*)ws, out, (hipStream_t)stream);
    if (rc != TRACE_OK) return fail(rc, "score_rows launch failed (R, K % 64, ld / ldw % 8 or head widths out of range)");
    return TRACE_OK;
}
static int score_buffers(trace_ctx* c) {
    const size_t PR = pf_rows(c->max_ctx);
    if (!c->score_ws) TRY(dalloc(c, &c->score_ws, score_ws_floats((int)PR, c->V)));
    if (!c->d_score_heads) TRY(dalloc(c, &c->d_score_heads, PR));
    if (!c->d_score_ids) TRY(dalloc(c, &c->d_score_ids, PR));
    if (!c->d_score_out) TRY(dalloc(c, &c->d_score_out, PR));
    return TRACE_OK;
}
extern "C" int trace_llm_score_rows(trace_ctx* c, const void* hidden, int R, const int32_t* heads, const int32_t* ids, float* out, void* stream) {
    if (!c || !c->finalized) return fail(TRACE_ERR_STATE, "context not finalized");
    if (!hidden || !heads || !ids || !out) return fail(TRACE_ERR_ARG, "null pointer");
    if (R < 1 || (size_t)R > pf_rows(c->max_ctx)) return fail(TRACE_ERR_ARG, "R outside 1 .. the prefill workspace's rows");
    TRY(score_buffers(c));
    const int rc = launch_score_rows((const bf16_t*)hidden, c->H, c->wheads, c->H, c->H, R, heads, ids, c->V, c->Tv, c->Sv, c->score_ws, out, (hipStream_t)stream);
    if (rc != TRACE_OK) return fail(rc, "score_rows launch failed");
    return TRACE_OK;
}
// trace_llm_prefill_append's pass (prefill_entry) with every row's final-norm hidden state kept, then the score of the n x L rows.  Everything is
// checked before the first launch.
extern "C" int trace_llm_score_append(trace_ctx* c, int slot0, int n, int past, const void* const* embeds, int L, const int32_t* heads, const int32_t* ids,
                                      float* out, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    int M = 0;
    TRY(prefill_entry(c, slot0, n, past, embeds, L, nullptr, stream, -1, true, [&] {
        if (!heads || !ids || !out) return fail(TRACE_ERR_ARG, "null heads / ids / out");
        M = n * L;
        for (int i = 0; i < M; ++i) {
            if (heads[i] < 0 || heads[i] > 2) return fail(TRACE_ERR_ARG, "head must be 0, 1 or 2");
            if (ids[i] < -1 || ids[i] >= c->NV) return fail(TRACE_ERR_ARG, "id must be -1 (ignore) or a vocabulary id");
        }
        TRY(score_buffers(c));
        HIPCHK(hipMemcpyAsync(c->d_score_heads, heads, (size_t)M * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(c->d_score_ids, ids, (size_t)M * 4, hipMemcpyHostToDevice, s));
        return (int)TRACE_OK;
    }));
    const int rc = launch_score_rows(c->pH, c->H, c->wheads, c->H, c->H, M, c->d_score_heads, c->d_score_ids, c->V, c->Tv, c->Sv, c->score_ws, c->d_score_out, s);
    if (rc != TRACE_OK) return fail(rc, "score_rows launch failed");
    HIPCHK(hipMemcpyAsync(out, c->d_score_out, (size_t)M * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return TRACE_OK;
}

extern "C" int trace_op_sample(const float* logits, int ld, int B, const int32_t* heads, int V, int Tv, int Sv, float T, int top_k, float top_p,
                               uint64_t seed, const int32_t* steps, int32_t* out_ids, void* stream) {
    if (!logits || !heads || !steps || !out_ids) return fail(TRACE_ERR_ARG, "null pointer");
    if (const char* m = sampling_bad(T, top_k, top_p)) return fail(TRACE_ERR_ARG, m);
    const int rc = launch_sample_rows(logits, ld, B, heads, V, Tv, Sv, make_sampling(T, top_k, top_p, seed), steps, out_ids, (hipStream_t)stream);
    if (rc != TRACE_OK) return fail(rc, "sample launch failed (B, ld or head widths out of range)");
    return TRACE_OK;
}

extern "C" int trace_op_sample_ex(const float* logits, int ld, int B, const int32_t* heads, int V, int Tv, int Sv, const trace_sampling* t,
                                  const int32_t* steps, int32_t* out_ids, void* stream) {
    if (!logits || !heads || !steps || !out_ids) return fail(TRACE_ERR_ARG, "null pointer");
    if (const char* m = sampling_struct_bad(t)) return fail(TRACE_ERR_ARG, m);
    if (const char* m = sampling_domain_bad(*t)) return fail(TRACE_ERR_ARG, m);
    const int rc = launch_sample_rows(logits, ld, B, heads, V, Tv, Sv, make_sampling(*t), steps, out_ids, (hipStream_t)stream);
    if (rc != TRACE_OK) return fail(rc, "sample launch failed (B, ld or head widths out of range)");
    return TRACE_OK;
}

extern "C" int trace_decode_host_mode(trace_ctx* c, int on) {
    if (!c) return fail(TRACE_ERR_ARG, "null ctx");
    c->host_mode = on ? 1 : 0;
    return TRACE_OK;
}

extern "C" int trace_decode_feed(trace_ctx* c, const int32_t* tokens, int B, void* stream) {
    if (!c || c->B < 1 || !c->host_mode) return fail(TRACE_ERR_STATE, "trace_decode_feed needs host-select mode and an active batch");
    if (!tokens || B != c->B) return fail(TRACE_ERR_ARG, "bad tokens / B");
    if (c->fed >= c->max_new) return fail(TRACE_ERR_STATE, "max_new tokens already fed");
    hipStream_t s = (hipStream_t)stream;
    for (int b = 0; b < B; ++b) {
        if (tokens[b] < 0 || tokens[b] >= c->NV) return fail(TRACE_ERR_ARG, "token id out of range");
        HIPCHK(hipMemcpyAsync(c->d_forced + (size_t)b * c->max_new + c->fed, tokens + b, 4, hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    TRY(select_only(c, SELECT_TILES, nullptr, c->fed > 0 ? 1 : 0, s));
    c->fed += 1;
    return TRACE_OK;
}

// ------------------------------------------------------------------------------------------------ pipeline streams
extern "C" int trace_stream_create(trace_ctx* c, int cu_first, int cu_count, void** stream_out) {
    if (!c || !stream_out) return fail(TRACE_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(c->dev));
    hipStream_t s = nullptr;
    if (cu_count == 0) {
        HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    } else {
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, c->dev));
        const int ncu = prop.multiProcessorCount;
        if (cu_first < 0 || cu_count < 8 || (cu_first % 8) || (cu_count % 8) || cu_first + cu_count > ncu)
            return fail(TRACE_ERR_ARG, "CU range must be multiples of 8 (one CU per XCD) inside the device's " + std::to_string(ncu) + " CUs");
        std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
        for (int i = cu_first; i < cu_first + cu_count; ++i) mask[i / 32] |= 1u << (i % 32);
        HIPCHK(hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()));
    }
    if (gemm_pers_init(s) != TRACE_OK) { hipStreamDestroy(s); return fail(TRACE_ERR_HIP, "persistent GEMM ticket counters"); }
    if (cu_count > 0) gemm_pers_set_cap(s, cu_count);          // a CU-masked stream: its persistent GEMMs launch one workgroup per CU IT can use
    c->streams.push_back(s);
    *stream_out = (void*)s;
    return TRACE_OK;
}
extern "C" int trace_stream_destroy(trace_ctx* c, void* stream) {
    if (!c || !stream) return fail(TRACE_ERR_ARG, "null argument");
    auto it = std::find(c->streams.begin(), c->streams.end(), (hipStream_t)stream);
    if (it == c->streams.end()) return fail(TRACE_ERR_ARG, "not a stream of this context");
    HIPCHK(hipSetDevice(c->dev));
    HIPCHK(hipStreamSynchronize(*it));
    gemm_pers_forget(*it);
    HIPCHK(hipStreamDestroy(*it));
    c->streams.erase(it);
    return TRACE_OK;
}
extern "C" int trace_set_gemm_cus(trace_ctx* c, int n) {
    if (!c || n < 0) return fail(TRACE_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(c->dev));
    // per stream, and only this context's streams (trace_stream_create already sets a CU-masked stream's cap to its CU count; this overrides it).
    // Until round 3 this wrote a process-wide number that nothing reset: every later persistent GEMM of the process stayed capped.
    for (hipStream_t st : c->streams)
        if (gemm_pers_set_cap(st, n) != TRACE_OK) return fail(TRACE_ERR_HIP, "persistent GEMM ticket counters");
    return TRACE_OK;
}

// debugging aid (tools/pipeline_stress.py): device addresses and element strides of the KV caches and of the prefill's last-position hidden rows
extern "C" int trace_debug_buffers(trace_ctx* c, void** kcache, void** vcache, void** xlast, int64_t* strides) {
    if (!c || !kcache || !vcache || !xlast || !strides) return fail(TRACE_ERR_ARG, "null argument");
    if (c->kv8) return fail(TRACE_ERR_STATE, "this context keeps an e4m3 KV cache: trace_debug_kv8_buffers");
    *kcache = c->kcache; *vcache = c->vcache; *xlast = c->xlast;
    strides[0] = (int64_t)c->layer_stride; strides[1] = (int64_t)c->slot_stride; strides[2] = (int64_t)c->kv_head_stride; strides[3] = c->ctx_pad;
    strides[4] = c->NL; strides[5] = c->NKV; strides[6] = c->HD; strides[7] = c->H;
    return TRACE_OK;
}
extern "C" int trace_debug_kv8_buffers(trace_ctx* c, void** k8, void** v8, void** ks, void** vs, int64_t* strides) {
    if (!c || !k8 || !v8 || !ks || !vs || !strides) return fail(TRACE_ERR_ARG, "null argument");
    if (!c->kv8) return fail(TRACE_ERR_STATE, "this context keeps a 16-bit KV cache: trace_debug_buffers");
    *k8 = c->k8cache; *v8 = c->v8cache; *ks = c->kscache; *vs = c->vscache;
    strides[0] = (int64_t)c->layer_stride; strides[1] = (int64_t)c->slot_stride; strides[2] = (int64_t)c->kv_head_stride; strides[3] = c->ctx_pad;
    strides[4] = c->NL; strides[5] = c->NKV; strides[6] = c->HD; strides[7] = c->H;
    return TRACE_OK;
}

extern "C" int trace_set_profile(trace_ctx* c, int on) {
    if (!c) return fail(TRACE_ERR_ARG, "null ctx");
    c->profile = on; c->bracket_kind = 0; c->ksum_ms = 0.0; c->ksamples = 0; c->kev_used = 0; c->kbytes_sum = 0.0; c->msum_ms = 0.0; c->msamples = 0; c->mM = 0;
    return TRACE_OK;
}
extern "C" int trace_set_profile_brackets(trace_ctx* c, int mask) {
    if (!c) return fail(TRACE_ERR_ARG, "null ctx");
    c->bracket_mask = mask & 15;
    return TRACE_OK;
}
extern "C" int trace_get_profile(trace_ctx* c, float* out, int n) {
    if (!c || !out) return fail(TRACE_ERR_ARG, "null argument");
    for (int i = 0; i < n && i < 20; ++i) out[i] = c->prof[i];
    return TRACE_OK;
}

// ------------------------------------------------------------------------------------------------ op-level hooks
extern "C" int trace_op_gemm(const void* A, int lda, const void* W, int ldw, void* C, int ldc, const void* bias, const void* R,
                             int ldr, int M, int N, int K, int epilogue, void* stream) {
    return gemm((const bf16_t*)A, lda, (const bf16_t*)W, ldw, (bf16_t*)C, ldc, (const bf16_t*)bias, (const bf16_t*)R, ldr, M, N, K,
                epilogue, (hipStream_t)stream);
}
extern "C" int trace_op_layernorm(const void* x, void* y, const void* w, const void* b, int rows, int D, float eps, void* stream) {
    LCHK(launch_layernorm((const bf16_t*)x, D, (bf16_t*)y, D, (const bf16_t*)w, (const bf16_t*)b, rows, D, eps, (hipStream_t)stream));
    return TRACE_OK;
}
extern "C" int trace_op_rmsnorm(const void* x, void* y, const void* w, int rows, int D, float eps, void* stream) {
    LCHK(launch_rmsnorm((const bf16_t*)x, D, (bf16_t*)y, D, (const bf16_t*)w, rows, D, eps, (hipStream_t)stream));
    return TRACE_OK;
}
// The norms with everything the engine's call sites use: row strides, the SiLU and residual tails of the LayerNorm (y may alias x or res)
extern "C" int trace_op_layernorm_ex(const void* x, int ldx, void* y, int ldy, const void* w, const void* b, int rows, int D, float eps, int silu,
                                     const void* res, int ldres, void* stream) {
    if (!x || !y || !w || !b) return fail(TRACE_ERR_ARG, "null argument");
    LCHK(launch_layernorm((const bf16_t*)x, ldx, (bf16_t*)y, ldy, (const bf16_t*)w, (const bf16_t*)b, rows, D, eps, (hipStream_t)stream, silu,
                          (const bf16_t*)res, ldres));
    return TRACE_OK;
}
extern "C" int trace_op_rmsnorm_ex(const void* x, int ldx, void* y, int ldy, const void* w, int rows, int D, float eps, void* stream) {
    if (!x || !y || !w) return fail(TRACE_ERR_ARG, "null argument");
    LCHK(launch_rmsnorm((const bf16_t*)x, ldx, (bf16_t*)y, ldy, (const bf16_t*)w, rows, D, eps, (hipStream_t)stream));
    return TRACE_OK;
}
// The STC connector's row kernels (stc.hip), each alone on loose tensors, as stc_block / trace_stc_connector call them.  Every refusal comes before any launch.
extern "C" int trace_op_dwconv3x3(const void* x, const void* w, void* y, int N, int H, int W, int C, void* stream) {
    if (!x || !w || !y) return fail(TRACE_ERR_ARG, "null argument");
    if (N < 1 || H < 1 || W < 1 || C < 8 || C % 8) return fail(TRACE_ERR_ARG, "dwconv3x3: N, H, W >= 1 and C a positive multiple of 8");
    LCHK(launch_dwconv3x3((const bf16_t*)x, (const bf16_t*)w, (bf16_t*)y, N, H, W, C, (hipStream_t)stream));
    return TRACE_OK;
}
extern "C" int trace_op_avgpool(const void* x, void* y, int N, int HW, int C, void* stream) {
    if (!x || !y) return fail(TRACE_ERR_ARG, "null argument");
    if (N < 1 || N > 65535 || HW < 1 || C < 64 || C % 64) return fail(TRACE_ERR_ARG, "avgpool: 1 <= N <= 65535, HW >= 1 and C a positive multiple of 64");
    LCHK(launch_avgpool((const bf16_t*)x, (bf16_t*)y, N, HW, C, (hipStream_t)stream));
    return TRACE_OK;
}
extern "C" int trace_op_bias_act(void* x, const void* bias, int64_t rows, int C, int act, void* stream) {
    if (!x) return fail(TRACE_ERR_ARG, "null argument");
    if (rows < 1 || C < 8 || C % 8) return fail(TRACE_ERR_ARG, "bias_act: rows >= 1 and C a positive multiple of 8");
    if (act < ACT_NONE || act > ACT_GELU) return fail(TRACE_ERR_ARG, "bias_act: act is 0 (none), 1 (SiLU), 2 (sigmoid) or 3 (GELU)");
    LCHK(launch_bias_act((bf16_t*)x, (const bf16_t*)bias, (long)rows, C, act, (hipStream_t)stream));
    return TRACE_OK;
}
extern "C" int trace_op_scale_rows(void* x, const void* gate, int N, int HW, int C, void* stream) {
    if (!x || !gate) return fail(TRACE_ERR_ARG, "null argument");
    if (N < 1 || HW < 1 || C < 8 || C % 8) return fail(TRACE_ERR_ARG, "scale_rows: N, HW >= 1 and C a positive multiple of 8");
    LCHK(launch_scale_rows((bf16_t*)x, (const bf16_t*)gate, N, HW, C, (hipStream_t)stream));
    return TRACE_OK;
}
extern "C" int trace_op_im2col3d(const void* x, void* A, int T, int H, int W, int C, void* stream) {
    if (!x || !A) return fail(TRACE_ERR_ARG, "null argument");
    if (T < 1 || H < 1 || W < 1 || C < 8 || C % 8) return fail(TRACE_ERR_ARG, "im2col3d: T, H, W >= 1 and C a positive multiple of 8");
    LCHK(launch_im2col3d((const bf16_t*)x, (bf16_t*)A, T, H, W, C, T / 2 + 1, H / 2 + 1, W / 2 + 1, (hipStream_t)stream));
    return TRACE_OK;
}
extern "C" int trace_op_permute_conv3d_w(const void* w, void* out, int Co, int Ci, void* stream) {
    if (!w || !out) return fail(TRACE_ERR_ARG, "null argument");
    if (Co < 1 || Ci < 1) return fail(TRACE_ERR_ARG, "permute_conv3d_w: Co, Ci >= 1");
    LCHK(launch_permute_conv3d_w((const bf16_t*)w, (bf16_t*)out, Co, Ci, (hipStream_t)stream));
    return TRACE_OK;
}
// launch_slot_pool alone (no readout GEMM): res_out [T, 8, D].  ws: trace_op_slot_pool_ws_floats(T, D) floats.
extern "C" int64_t trace_op_slot_pool_ws_floats(int T, int D) { return T > 0 && D > 0 ? (int64_t)launch_slot_pool_ws_floats(T, D) : (int64_t)TRACE_ERR_ARG; }
extern "C" int trace_op_slot_pool(const void* feats, int64_t frame_stride, int row_stride, const void* ln_w, const void* ln_b, const void* slots,
                                  const float* cos_t, const float* sin_t, void* res_out, int T, int n, int D, float eps, float* ws, int64_t ws_floats,
                                  void* stream) {
    if (!feats || !ln_w || !ln_b || !slots || !cos_t || !sin_t || !res_out) return fail(TRACE_ERR_ARG, "null argument");
    if (frame_stride < 0 || (frame_stride % 8) || row_stride < D) return fail(TRACE_ERR_ARG, "strides: frame_stride a multiple of 8 elements, row_stride >= D");
    if (ws_floats < 0) return fail(TRACE_ERR_ARG, "bad workspace size");
    LCHK(launch_slot_pool((const bf16_t*)feats, (long)frame_stride, row_stride, (const bf16_t*)ln_w, (const bf16_t*)ln_b, (const bf16_t*)slots, cos_t, sin_t,
                          (bf16_t*)res_out, T, n, D, 8, eps, ws, (size_t)ws_floats, (hipStream_t)stream));
    return TRACE_OK;
}
// The fused ViT front end from checkpoint-layout tensors, as trace_ctx_finalize + trace_vit_forward run it: launch_patch_pack, launch_cls_row, launch_patch_embed.
// conv_w [D, 3 P P], cls [D], pos [G G + 1, D], X_out [T, G G + 1, D]; ws: trace_op_patch_embed_ws_elems(P, D) 16-bit elements (packed weight + CLS row).
extern "C" int64_t trace_op_patch_embed_ws_elems(int P, int D) {
    return patch_embed_supported(P, P, D) ? (int64_t)(patch_embed_packed_elems(P, D) + (size_t)D) : (int64_t)TRACE_ERR_ARG;
}
extern "C" int trace_op_patch_embed(const void* frames, int frames_dtype, const void* conv_w, const void* cls, const void* pos, const void* pre_w,
                                    const void* pre_b, void* X_out, int T, int S, int P, int D, float eps, void* ws, int64_t ws_elems, void* stream) {
    if (!frames || !conv_w || !cls || !pos || !pre_w || !pre_b || !X_out) return fail(TRACE_ERR_ARG, "null argument");
    if (T < 1 || S < 1 || !patch_embed_supported(S, P, D)) return fail(TRACE_ERR_ARG, "geometry the fused front end does not take (P in {14, 16}, S % P == 0, D in {128, 256, 512, 1024})");
    if (frames_dtype != 0 && frames_dtype != 1) return fail(TRACE_ERR_ARG, "frames_dtype: 0 = 16-bit, 1 = fp32");
    if (!ws || ws_elems < trace_op_patch_embed_ws_elems(P, D)) return fail(TRACE_ERR_ARG, "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    bf16_t* wp = (bf16_t*)ws;
    bf16_t* cls_row = wp + patch_embed_packed_elems(P, D);
    LCHK(launch_patch_pack((const bf16_t*)conv_w, 3 * P * P, wp, D, P, s));
    LCHK(launch_cls_row((const bf16_t*)cls, (const bf16_t*)pos, (const bf16_t*)pre_w, (const bf16_t*)pre_b, cls_row, D, eps, s));
    LCHK(launch_patch_embed(frames, frames_dtype == 1, wp, (const bf16_t*)pos, (const bf16_t*)pre_w, (const bf16_t*)pre_b, cls_row, (bf16_t*)X_out, T, S, P, D,
                            eps, s));
    return TRACE_OK;
}
// Q [batch, nq, heads, hd], K/V [batch, nkv, kv_heads, hd] (token-major, heads interleaved), O like Q.
// vt_scratch: batch*kv_heads*hd*round_up(nkv,64) bf16.
extern "C" int trace_op_attention(const void* Q, const void* K, const void* V, void* O, void* vt_scratch, int batch, int heads,
                                  int kv_heads, int nq, int nkv, int head_dim, int causal, float scale, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const int pad = round_up(nkv, 64);
    AttnArgs a{};
    a.Q = (const bf16_t*)Q; a.K = (const bf16_t*)K; a.V = (const bf16_t*)vt_scratch; a.O = (bf16_t*)O;
    a.q_bs = (long)nq * heads * head_dim; a.q_hs = head_dim; a.q_rs = heads * head_dim;
    a.k_bs = (long)nkv * kv_heads * head_dim; a.k_hs = head_dim; a.k_rs = kv_heads * head_dim;
    a.v_bs = (long)kv_heads * head_dim * pad; a.v_hs = (long)head_dim * pad; a.v_rs = pad;
    a.o_bs = a.q_bs; a.o_hs = head_dim; a.o_rs = heads * head_dim;
    a.nq_rows = nq; a.nkv_rows = nkv; a.batch = batch; a.heads = heads; a.kv_heads = kv_heads; a.scale = scale; a.causal = causal;
    a.Vrow = (const bf16_t*)V; a.vr_bs = a.k_bs; a.vr_hs = head_dim; a.vr_rs = kv_heads * head_dim;
    a.v_perm = (head_dim == 64 && !causal && heads == kv_heads && attn_vit_wants_perm(nkv, true)) ? (attn_vit_rowmajor_v() ? 2 : 1) : 0;
    if (a.v_perm != 2)
        LCHK(launch_transpose_v((const bf16_t*)V, a.k_bs, head_dim, kv_heads * head_dim, (bf16_t*)vt_scratch, a.v_bs, a.v_hs, pad, nkv,
                                head_dim, kv_heads, batch, s, a.v_perm));
    if (head_dim == 64) { LCHK(launch_attn_vit(a, s)); }
    else if (head_dim == 128) { LCHK(launch_attn_prefill(a, s)); }
    else return fail(TRACE_ERR_ARG, "head_dim must be 64 or 128");
    return TRACE_OK;
}
// Decode GEMV test hooks.  w_tiled: W is in the decode tile layout (trace_op_tile_pack) instead of row-major [N][K].
// epilogue 4 (EPI_PARTIAL): `out` receives the fp32 partial rows [trace_op_skinny_ks(...)][64][N] instead of bf16.
static float* g_sk_ws = nullptr;
static unsigned int* g_sk_tk = nullptr;
static size_t g_sk_ws_floats = 0;
static int g_sk_ntk = 0;
extern "C" int trace_op_skinny_gemm(const void* X, const void* W, void* out, const void* R, int B, int N, int K, int epilogue,
                                    int w_tiled, void* stream) {
    const int No = epilogue == EPI_SWIGLU ? N / 2 : N;
    const size_t need = skinny_ws_floats(N, K, epilogue);
    if (need > g_sk_ws_floats || N / 16 > g_sk_ntk) {             // grow-only scratch (never freed)
        HIPCHK(hipDeviceSynchronize());
        if (g_sk_ws) hipFree(g_sk_ws);
        if (g_sk_tk) hipFree(g_sk_tk);
        g_sk_ws_floats = std::max(need, g_sk_ws_floats) + 64; g_sk_ntk = std::max(N / 16, g_sk_ntk);
        HIPCHK(hipMalloc((void**)&g_sk_ws, g_sk_ws_floats * 4));
        HIPCHK(hipMalloc((void**)&g_sk_tk, (size_t)g_sk_ntk * 4));
        HIPCHK(hipMemset(g_sk_tk, 0, (size_t)g_sk_ntk * 4));
    }
    LCHK(launch_skinny_gemm((const bf16_t*)X, K, (const bf16_t*)W, K, (bf16_t*)out, No, (const bf16_t*)R, No, B, N, K, epilogue,
                            w_tiled, g_sk_ws, g_sk_ws_floats, g_sk_tk, g_sk_ntk, (hipStream_t)stream));
    if (epilogue == EPI_PARTIAL && out)
        HIPCHK(hipMemcpyAsync(out, g_sk_ws, (size_t)skinny_ks(SK_BF16, N, K, epilogue, B) * SK_ROWS * N * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return TRACE_OK;
}
extern "C" int trace_op_skinny_ks(int N, int K, int epilogue, int B) { return skinny_ks(SK_BF16, N, K, epilogue, B); }
extern "C" int trace_op_skinny_plan(int kind, int N, int K, int epilogue, int B, int64_t* out) {
    if (!out || kind < SK_BF16 || kind > SK_W8A16 || !skinny_shape_ok((SkinnyKind)kind, N, K, epilogue, B)) return fail(TRACE_ERR_ARG, "the decode GEMV of this kind does not take this shape");
    const SkinnyPlan p = skinny_plan((SkinnyKind)kind, N, K, epilogue, B);
    const int64_t v[11] = {p.KS, p.chunk_units, p.T, p.WPT, p.ntiles, p.grid, p.threads, p.NT, p.NB, (int64_t)p.lds_bytes, (int64_t)skinny_partial_floats((SkinnyKind)kind, N, K)};
    std::copy(v, v + 11, out);
    return TRACE_OK;
}
extern "C" int trace_op_decode_route(int B, int fp8_scheme, int H, int I, int QKV, int32_t* out) {
    if (!out || B < 1 || B > SK_ROWS || fp8_scheme < 0 || fp8_scheme > 2 || (fp8_scheme && B > SKINNY_ROWS)) return fail(TRACE_ERR_ARG, "bad batch or fp8 scheme");
    if (H < 128 || I < 128 || QKV < 16) return fail(TRACE_ERR_ARG, "bad geometry");
    const DecodeRoute r = decode_route(B, fp8_scheme, H, I, QKV, g_tune);
    const int32_t v[8] = {r.step, (int32_t)r.kind, r.qkv_finish, r.ks_q, r.ks_o, r.ks_g, r.ks_d, r.nsplit};
    std::copy(v, v + 8, out);
    return TRACE_OK;
}
// the same two for w4 weights (the older entry points keep refusing kind / scheme 3)
extern "C" int trace_op_skinny_w4_plan(int N, int K, int B, int64_t* out) {
    if (!out || !skinny_shape_ok(SK_W4A16, N, K, EPI_PARTIAL, B)) return fail(TRACE_ERR_ARG, "the w4 decode GEMV does not take this shape (K % 256, N % 16, B <= 64)");
    const SkinnyPlan p = skinny_plan(SK_W4A16, N, K, EPI_PARTIAL, B);
    const int64_t v[11] = {p.KS, p.chunk_units, p.T, p.WPT, p.ntiles, p.grid, p.threads, p.NT, p.NB, (int64_t)p.lds_bytes, (int64_t)skinny_partial_floats(SK_W4A16, N, K)};
    std::copy(v, v + 11, out);
    return TRACE_OK;
}
extern "C" int trace_op_decode_route_w4(int B, int H, int I, int QKV, int32_t* out) {
    if (!out || B < 1 || B > SKINNY_ROWS) return fail(TRACE_ERR_ARG, "bad batch (w4 weights decode at most 64 sequences together)");
    if (H < 256 || I < 256 || H % 256 || I % 256 || QKV < 16 || QKV % 16) return fail(TRACE_ERR_ARG, "bad geometry");
    const DecodeRoute r = decode_route(B, 3, H, I, QKV, g_tune);
    const int32_t v[8] = {r.step, (int32_t)r.kind, r.qkv_finish, r.ks_q, r.ks_o, r.ks_g, r.ks_d, r.nsplit};
    std::copy(v, v + 8, out);
    return TRACE_OK;
}
extern "C" int trace_op_sk_rows(void) { return SK_ROWS; }
// gate|up of a wide decode step: X [M <= 128, K] . Wt (the 16-row interleaved gate|up matrix in the decode tile layout) -> SwiGLU -> out [M, N/2] bf16
extern "C" int trace_op_gemm_swiglu_tiled(const void* X, const void* Wt, void* out, int M, int N, int K, int ring, void* stream) {
    GemmArgs g{(const bf16_t*)X, K, (const bf16_t*)Wt, K, (bf16_t*)out, N / 2, nullptr, nullptr, 0, M, N, K, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, ring ? 5 : 1};
    return gemm_checked(g, EPI_SWIGLU, (hipStream_t)stream, "tiled SwiGLU GEMM");
}
// [M <= 128, K] x [N, K]^T as fp32 k-chunk partial rows [trace_op_gemm_partial_ks(N, K)][trace_op_sk_rows()][N] (decode batches above 64 rows)
extern "C" int trace_op_gemm_partial_ks(int N, int K) { return gemm_partial_ks(N, K); }
extern "C" int trace_op_gemm_partial(const void* A, const void* W, float* part, int M, int N, int K, int w_tiled, void* stream) {
    GemmArgs g{(const bf16_t*)A, K, (const bf16_t*)W, K, nullptr, 0, nullptr, nullptr, 0, M, N, K, nullptr, 0, nullptr, nullptr, 0, part, gemm_partial_ks(N, K), w_tiled};
    return gemm_checked(g, EPI_PARTIAL, (hipStream_t)stream, "partial GEMM");
}
// ---- fp8 path hooks (tests/test_gpu_fp8.py) ----
extern "C" int trace_op_quant_rows_fp8(const void* X, void* X8, float* sx, int rows, int K, void* stream) {
    LCHK(launch_quant_rows_fp8((const bf16_t*)X, K, (uint8_t*)X8, K, sx, rows, K, (hipStream_t)stream));
    return TRACE_OK;
}
extern "C" int trace_op_gemm_fp8(const void* A8, const float* sa, const void* W8, const float* sw, void* C, const void* R, int M, int N, int K,
                                 int epilogue, void* stream) {
    const int No = epilogue == EPI_SWIGLU ? N / 2 : N;
    GemmArgs g{(const bf16_t*)A8, K, (const bf16_t*)W8, K, (bf16_t*)C, No, nullptr, (const bf16_t*)R, No, M, N, K, nullptr, 1, sa, sw};
    return gemm_checked(g, epilogue, (hipStream_t)stream, "fp8 gemm");
}
// X [B,K] (e4m3 bytes + sx, or bf16 with sx null: the weight-only form), W8 [N,K] e4m3 row-major + sw -> out fp32 [B,N] (the k-chunk partial rows summed
// here, in chunk order)
static int op_skinny_e4m3(const void* X, const float* sx, const void* W8, const float* sw, float* out, int B, int N, int K, hipStream_t s) {
    static uint8_t* wt = nullptr; static size_t wt_bytes = 0;
    static float* ws = nullptr; static size_t ws_floats = 0;
    const int KS = skinny_ks(sx ? SK_W8A8 : SK_W8A16, N, K, EPI_PARTIAL, B);
    const size_t need_w = (size_t)N * K, need_ws = (size_t)KS * SK_ROWS * N;
    if (need_w > wt_bytes) { HIPCHK(hipDeviceSynchronize()); if (wt) hipFree(wt); HIPCHK(hipMalloc((void**)&wt, need_w)); wt_bytes = need_w; }
    if (need_ws > ws_floats) { HIPCHK(hipDeviceSynchronize()); if (ws) hipFree(ws); HIPCHK(hipMalloc((void**)&ws, need_ws * 4)); ws_floats = need_ws; }
    LCHK(launch_tile_pack_fp8((const uint8_t*)W8, K, wt, N, K, s));
    if (sx) LCHK(launch_skinny_fp8((const uint8_t*)X, K, sx, wt, sw, B, N, K, ws, ws_floats, s));
    else LCHK(launch_skinny_w8((const bf16_t*)X, K, wt, sw, B, N, K, ws, ws_floats, s));
    std::vector<float> h((size_t)KS * SK_ROWS * N), o((size_t)B * N, 0.f);
    HIPCHK(hipMemcpyAsync(h.data(), ws, h.size() * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int ks = 0; ks < KS; ++ks)
        for (int b = 0; b < B; ++b)
            for (int n = 0; n < N; ++n) o[(size_t)b * N + n] += h[((size_t)ks * SK_ROWS + b) * N + n];
    HIPCHK(hipMemcpy(out, o.data(), o.size() * 4, hipMemcpyHostToDevice));
    return TRACE_OK;
}
extern "C" int trace_op_skinny_fp8(const void* X8, const float* sx, const void* W8, const float* sw, float* out, int B, int N, int K, void* stream) {
    if (!sx) return fail(TRACE_ERR_ARG, "null activation scales");
    return op_skinny_e4m3(X8, sx, W8, sw, out, B, N, K, (hipStream_t)stream);
}
extern "C" int trace_op_skinny_w8(const void* X, const void* W8, const float* sw, float* out, int B, int N, int K, void* stream) {
    return op_skinny_e4m3(X, nullptr, W8, sw, out, B, N, K, (hipStream_t)stream);
}

// ---- w4 path hooks (tests/test_gpu_w4.py) ----
#define W4_BF16_ONLY() do { if (TRACE_ELEMENT_TYPE != 0) return fail(TRACE_ERR_ARG, "the w4 kernels need the bf16 library"); } while (0)
extern "C" int trace_op_quant_rows_w4(const void* W, void* codes, void* exps, int N, int K, void* stream) {
    W4_BF16_ONLY();
    if (!W || !codes || !exps) return fail(TRACE_ERR_ARG, "null argument");
    LCHK(launch_quant_rows_w4((const bf16_t*)W, K, (uint8_t*)codes, (uint8_t*)exps, N, K, (hipStream_t)stream));
    return TRACE_OK;
}
extern "C" int trace_op_tile_pack_w4(const void* codes, const void* exps, void* tcodes, void* texps, int N, int K, void* stream) {
    W4_BF16_ONLY();
    if (!codes || !exps || !tcodes || !texps) return fail(TRACE_ERR_ARG, "null argument");
    LCHK(launch_tile_pack_w4((const uint8_t*)codes, (const uint8_t*)exps, (uint8_t*)tcodes, (uint8_t*)texps, N, K, 0, 1, (hipStream_t)stream));
    return TRACE_OK;
}
extern "C" int trace_op_dequant_w4(const void* tcodes, const void* texps, void* out, int N, int K, void* stream) {
    W4_BF16_ONLY();
    if (!tcodes || !texps || !out) return fail(TRACE_ERR_ARG, "null argument");
    LCHK(launch_dequant_w4((const uint8_t*)tcodes, (const uint8_t*)texps, (bf16_t*)out, K, N, K, (hipStream_t)stream));
    return TRACE_OK;
}
extern "C" int trace_op_skinny_w4(const void* X, const void* tcodes, const void* texps, float* out, int B, int N, int K, void* stream) {
    W4_BF16_ONLY();
    if (!X || !tcodes || !texps || !out) return fail(TRACE_ERR_ARG, "null argument");
    if (!skinny_shape_ok(SK_W4A16, N, K, EPI_PARTIAL, B)) return fail(TRACE_ERR_ARG, "the w4 decode GEMV does not take this shape (K % 256, N % 16, B <= 64)");
    const size_t floats = (size_t)skinny_ks(SK_W4A16, N, K, EPI_PARTIAL, B) * SK_ROWS * N;
    LCHK(launch_skinny_w4((const bf16_t*)X, K, (const uint8_t*)tcodes, (const uint8_t*)texps, B, N, K, out, floats, (hipStream_t)stream));
    return TRACE_OK;
}

// the fused-norm decode GEMV of small batches: part_in [ks_in][sk_rows][K] fp32 + R [B,K] -> xout [B,K] (new residual), out = fp32 partial rows
// [trace_op_skinny_ks(N,K,4,B)][sk_rows][N] of RMSNorm(xout; w) . W^T (W row-major here; packed internally)
extern "C" int trace_op_skinny_fused_norm(const float* part_in, int ks_in, const void* R, void* xout, const void* w, float eps, const void* W, float* out,
                                          int B, int N, int K, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!skinny_fused_norm_ok(N, K, B)) return fail(TRACE_ERR_ARG, "shape not supported by the fused-norm GEMV");
    bf16_t* wt = nullptr; float* ws = nullptr;
    const size_t wsf = skinny_ws_floats(N, K, EPI_PARTIAL);
    HIPCHK(hipMalloc((void**)&wt, (size_t)N * K * 2)); HIPCHK(hipMalloc((void**)&ws, wsf * 4));
    int rc = launch_tile_pack((const bf16_t*)W, K, wt, N, K, s);
    if (rc == TRACE_OK) rc = launch_skinny_gemm_fused_norm(part_in, ks_in, (const bf16_t*)R, K, (bf16_t*)xout, K, (const bf16_t*)w, eps, wt, B, N, K, ws, wsf, s);
    if (rc == TRACE_OK && hipMemcpyAsync(out, ws, (size_t)skinny_ks(SK_BF16, N, K, EPI_PARTIAL, B) * SK_ROWS * N * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) rc = TRACE_ERR_HIP;
    hipStreamSynchronize(s);
    hipFree(wt); hipFree(ws);
    if (rc != TRACE_OK) return fail(rc, "fused-norm GEMV failed");
    return TRACE_OK;
}

extern "C" int trace_op_tile_pack(const void* W, void* Wt, int N, int K, void* stream) {
    LCHK(launch_tile_pack((const bf16_t*)W, K, (bf16_t*)Wt, N, K, (hipStream_t)stream));
    return TRACE_OK;
}
extern "C" int trace_op_swiglu_combine(const float* part, int KS, int N2, void* out, int B, void* stream) {
    LCHK(launch_swiglu_combine(part, KS, N2, (bf16_t*)out, N2 / 2, B, (hipStream_t)stream));
    return TRACE_OK;
}
extern "C" int trace_op_add_rmsnorm(const float* part, int KS, const void* R, void* xout, const void* w, void* y, int B, int N,
                                    float eps, void* stream) {
    LCHK(launch_add_rmsnorm(part, KS, (const bf16_t*)R, N, (bf16_t*)xout, N, (const bf16_t*)w, (bf16_t*)y, N, B, N, eps,
                            (hipStream_t)stream));
    return TRACE_OK;
}
// the same launcher with everything the decode step passes it: row strides, xout == R, the e4m3 copy of y (y8 / sy) and an explicit chunk count
extern "C" int trace_op_add_rmsnorm_ex(const float* part, int KS, const void* R, int ldr, void* xout, int ldx, const void* w, void* y, int ldy, void* y8,
                                       float* sy, int B, int N, float eps, void* stream) {
    if (!part || !R || !xout || !w || !y) return fail(TRACE_ERR_ARG, "null argument");
    if ((y8 == nullptr) != (sy == nullptr)) return fail(TRACE_ERR_ARG, "y8 and sy go together");
    if (y8 && TRACE_ELEMENT_TYPE != 0) return fail(TRACE_ERR_ARG, "y8 / sy need the bf16 library (the fp16 build has no fp8 weight path)");
    if (N < 4 || ldr < N || ldx < N || ldy < N) return fail(TRACE_ERR_ARG, "row strides below N");
    LCHK(launch_add_rmsnorm(part, KS, (const bf16_t*)R, ldr, (bf16_t*)xout, ldx, (const bf16_t*)w, (bf16_t*)y, ldy, B, N, eps, (hipStream_t)stream,
                            (uint8_t*)y8, sy));
    return TRACE_OK;
}
// the SwiGLU-prologue decode GEMV of small batches: part_gu [ks_gu][sk_rows][2 K] fp32 -> out = fp32 partial rows [trace_op_skinny_ks(N,K,4,B)][sk_rows][N] of
// el(silu(sum gate) * sum up) . W^T (W row-major here; packed internally)
extern "C" int trace_op_skinny_fused_swiglu(const float* part_gu, int ks_gu, const void* W, float* out, int B, int N, int K, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!part_gu || !W || !out) return fail(TRACE_ERR_ARG, "null argument");
    if (B < 1 || B > 4 || ks_gu < 1 || !skinny_shape_ok(SK_BF16, N, K, EPI_PARTIAL, B)) return fail(TRACE_ERR_ARG, "shape not supported by the fused-SwiGLU GEMV");
    bf16_t* wt = nullptr; float* ws = nullptr;
    const size_t wsf = skinny_ws_floats(N, K, EPI_PARTIAL);
    HIPCHK(hipMalloc((void**)&wt, (size_t)N * K * 2));
    if (hipMalloc((void**)&ws, wsf * 4) != hipSuccess) { hipFree(wt); return fail(TRACE_ERR_HIP, "workspace allocation failed"); }
    int rc = launch_tile_pack((const bf16_t*)W, K, wt, N, K, s);
    if (rc == TRACE_OK) rc = launch_skinny_gemm_fused_swiglu(part_gu, ks_gu, wt, B, N, K, ws, wsf, s);
    if (rc == TRACE_OK && hipMemcpyAsync(out, ws, (size_t)skinny_ks(SK_BF16, N, K, EPI_PARTIAL, B) * SK_ROWS * N * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) rc = TRACE_ERR_HIP;
    hipStreamSynchronize(s);
    hipFree(wt); hipFree(ws);
    if (rc != TRACE_OK) return fail(rc, "fused-SwiGLU GEMV failed");
    return TRACE_OK;
}
// kcache [B, nkv, max_ctx, 128]; vtcache [B, nkv, 128, max_ctx] (V transposed; max_ctx % 32 == 0); pos[b] = index of the
// newest token (ctx = pos+1), already in the caches; q [B, nq*128] ready (rotated).  ws: B*nq*nsplit*130 floats.
// The identity slots and the ticket counters of the decode-attention hooks hold SK_ROWS rows x OP_ATTN_MAX_KV kv heads: a launch is refused unless it fits them.
constexpr int OP_ATTN_MAX_KV = 64;
static int32_t* g_op_slots = nullptr;
static unsigned int* g_op_tickets = nullptr;
static int op_attn_decode_state(int B, int nq, int nkv, int max_ctx, int nsplit) {
    if (B < 1 || B > SK_ROWS) return fail(TRACE_ERR_ARG, "bad batch (at most " + std::to_string(SK_ROWS) + " rows)");
    if (nkv < 1 || nkv > OP_ATTN_MAX_KV || nq != 4 * nkv || max_ctx < 32 || max_ctx % 32 || nsplit < 1) return fail(TRACE_ERR_ARG, "bad decode attention shape");
    if (!g_op_slots) {
        int32_t h[SK_ROWS];
        for (int i = 0; i < SK_ROWS; ++i) h[i] = i;
        HIPCHK(hipMalloc((void**)&g_op_slots, SK_ROWS * 4));
        HIPCHK(hipMemcpy(g_op_slots, h, SK_ROWS * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMalloc((void**)&g_op_tickets, SK_ROWS * OP_ATTN_MAX_KV * 4));
        HIPCHK(hipMemset(g_op_tickets, 0, SK_ROWS * OP_ATTN_MAX_KV * 4));
    }
    return TRACE_OK;
}
// slots[B] / pos[B] (device) as the appending hooks need them: every slot inside the caches, no slot twice, every position inside a slot.  Read back on
// `s` (the hooks are test entry points: one stream synchronisation per call), so nothing out of range ever reaches a launch.
static int op_check_slots_pos(const int32_t* slots, const int32_t* pos, int B, int num_slots, int max_ctx, hipStream_t s) {
    if (!slots || !pos || num_slots < 1) return fail(TRACE_ERR_ARG, "null slots / pos");
    std::vector<int32_t> hs(B), hp(B);
    HIPCHK(hipMemcpyAsync(hs.data(), slots, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hp.data(), pos, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::vector<char> seen(num_slots, 0);
    for (int b = 0; b < B; ++b) {
        if (hs[b] < 0 || hs[b] >= num_slots) return fail(TRACE_ERR_ARG, "slot out of range");
        if (seen[hs[b]]) return fail(TRACE_ERR_ARG, "slot given twice");
        seen[hs[b]] = 1;
        if (hp[b] < 0 || hp[b] >= max_ctx) return fail(TRACE_ERR_ARG, "position out of range");
    }
    return TRACE_OK;
}
extern "C" int trace_op_attn_decode(const void* q, const void* kcache, const void* vcache, const int32_t* pos, void* O, float* ws,
                                    int B, int nq, int nkv, int max_ctx, int nsplit, float scale, void* stream) {
    TRY(op_attn_decode_state(B, nq, nkv, max_ctx, nsplit));
    LCHK(launch_attn_decode((const bf16_t*)q, nq * 128, (bf16_t*)kcache, (bf16_t*)vcache, (long)nkv * max_ctx * 128,
                            (long)max_ctx * 128, max_ctx, g_op_slots, pos, (bf16_t*)O, nq * 128, ws, g_op_tickets, B, nq, nkv, 128, nsplit, scale, 0,
                            nullptr, nullptr, nullptr, 0, (hipStream_t)stream));
    return TRACE_OK;
}
// trace_op_attn_decode over caches of num_slots >= B slots (sequence b in slot b), positions below shared_rows (floored to a multiple of 32) of every
// sequence read from slot shared_slot; a sequence whose newest position lies below them is refused before the launch.
extern "C" int trace_op_attn_decode_shared(const void* q, const void* kcache, const void* vcache, const int32_t* pos, void* O, float* ws, int B, int nq,
                                           int nkv, int num_slots, int max_ctx, int nsplit, float scale, int shared_slot, int shared_rows, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!q || !kcache || !vcache || !O || !ws) return fail(TRACE_ERR_ARG, "null argument");
    TRY(op_attn_decode_state(B, nq, nkv, max_ctx, nsplit));
    if (num_slots < B || shared_rows < 0 || shared_rows > max_ctx) return fail(TRACE_ERR_ARG, "bad num_slots / shared_rows");
    shared_rows &= ~31;
    if (shared_rows > 0 && (shared_slot < 0 || shared_slot >= num_slots)) return fail(TRACE_ERR_ARG, "shared slot out of range");
    if (!pos) return fail(TRACE_ERR_ARG, "null pos");
    std::vector<int32_t> hp(B);
    HIPCHK(hipMemcpyAsync(hp.data(), pos, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int b = 0; b < B; ++b) {
        if (hp[b] < 0 || hp[b] >= max_ctx) return fail(TRACE_ERR_ARG, "position out of range");
        if (hp[b] < shared_rows) return fail(TRACE_ERR_ARG, "a sequence is shorter than the shared prefix");
    }
    LCHK(launch_attn_decode((const bf16_t*)q, nq * 128, (bf16_t*)kcache, (bf16_t*)vcache, (long)nkv * max_ctx * 128, (long)max_ctx * 128, max_ctx, g_op_slots,
                            pos, (bf16_t*)O, nq * 128, ws, g_op_tickets, B, nq, nkv, 128, nsplit, scale, 0, nullptr, nullptr, nullptr, 0, s,
                            shared_rows > 0 ? shared_slot : -1, shared_rows));
    return TRACE_OK;
}
extern "C" int trace_op_qkv_finish(const float* part, int ks, void* q_out, void* kcache, void* vtcache, const int32_t* slots, const int32_t* pos,
                                   const float* cos_t, const float* sin_t, int B, int nq, int nkv, int num_slots, int max_ctx, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!part || !q_out || !kcache || !vtcache || !cos_t || !sin_t || ks < 1) return fail(TRACE_ERR_ARG, "null argument");
    TRY(op_attn_decode_state(B, nq, nkv, max_ctx, 1));
    TRY(op_check_slots_pos(slots, pos, B, num_slots, max_ctx, s));
    LCHK(launch_qkv_finish(part, ks, (nq + 2 * nkv) * 128, (bf16_t*)q_out, (bf16_t*)kcache, (bf16_t*)vtcache, (long)nkv * max_ctx * 128, (long)max_ctx * 128,
                           max_ctx, slots, pos, B, nq, nkv, cos_t, sin_t, s));
    return TRACE_OK;
}
extern "C" int trace_op_attn_decode_fused(const float* part, int ks, void* kcache, void* vtcache, const int32_t* slots, const int32_t* pos,
                                          const float* cos_t, const float* sin_t, void* O, float* ws, int B, int nq, int nkv, int num_slots,
                                          int max_ctx, int nsplit, float scale, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!part || !kcache || !vtcache || !cos_t || !sin_t || !O || !ws || ks < 1) return fail(TRACE_ERR_ARG, "null argument");
    TRY(op_attn_decode_state(B, nq, nkv, max_ctx, nsplit));
    TRY(op_check_slots_pos(slots, pos, B, num_slots, max_ctx, s));
    LCHK(launch_attn_decode(nullptr, (nq + 2 * nkv) * 128, (bf16_t*)kcache, (bf16_t*)vtcache, (long)nkv * max_ctx * 128, (long)max_ctx * 128, max_ctx,
                            slots, pos, (bf16_t*)O, nq * 128, ws, g_op_tickets, B, nq, nkv, 128, nsplit, scale, 1, cos_t, sin_t, part, ks, s));
    return TRACE_OK;
}

// ---- e4m3 KV cache hooks (kv8.hip; tests/test_gpu_kv8_probes.py) ----
// loose arrays k8 [num_slots][nkv][max_ctx][128], v8 [num_slots][nkv][max_ctx/32][128][32], ks / vs [num_slots][nkv][max_ctx]
static Kv8Cache op_kv8(void* k8, void* v8, float* ks, float* vs, int nkv, int max_ctx) {
    return Kv8Cache{(uint8_t*)k8, (uint8_t*)v8, ks, vs, (long)nkv * max_ctx * 128, (long)max_ctx * 128, max_ctx};
}
static int op_check_pos(const int32_t* pos, int B, int max_ctx, hipStream_t s) {
    if (!pos) return fail(TRACE_ERR_ARG, "null pos");
    std::vector<int32_t> hp(B);
    HIPCHK(hipMemcpyAsync(hp.data(), pos, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int b = 0; b < B; ++b)
        if (hp[b] < 0 || hp[b] >= max_ctx) return fail(TRACE_ERR_ARG, "position out of range");
    return TRACE_OK;
}
static int op_check_slots(const int32_t* slots, int B, int num_slots, hipStream_t s) {
    if (!slots || num_slots < 1) return fail(TRACE_ERR_ARG, "null slots");
    std::vector<int32_t> hs(B);
    HIPCHK(hipMemcpyAsync(hs.data(), slots, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::vector<char> seen(num_slots, 0);
    for (int b = 0; b < B; ++b) {
        if (hs[b] < 0 || hs[b] >= num_slots) return fail(TRACE_ERR_ARG, "slot out of range");
        if (seen[hs[b]]) return fail(TRACE_ERR_ARG, "slot given twice");
        seen[hs[b]] = 1;
    }
    return TRACE_OK;
}
extern "C" int trace_op_attn_decode_kv8(const void* q, const void* k8, const void* v8, const float* ks, const float* vs, const int32_t* pos, void* O,
                                        float* ws, int B, int nq, int nkv, int max_ctx, int nsplit, float scale, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!q || !k8 || !v8 || !ks || !vs || !O || !ws) return fail(TRACE_ERR_ARG, "null argument");
    TRY(op_attn_decode_state(B, nq, nkv, max_ctx, nsplit));
    TRY(op_check_pos(pos, B, max_ctx, s));
    LCHK(launch_attn_decode_kv8((const bf16_t*)q, nq * 128, op_kv8((void*)k8, (void*)v8, (float*)ks, (float*)vs, nkv, max_ctx), g_op_slots, pos, (bf16_t*)O,
                                nq * 128, ws, g_op_tickets, B, nq, nkv, 128, nsplit, scale, s));
    return TRACE_OK;
}
extern "C" int trace_op_qkv_finish_kv8(const float* part, int ks_chunks, void* q_out, void* k8, void* v8, float* ks, float* vs, const int32_t* slots,
                                       const int32_t* pos, const float* cos_t, const float* sin_t, int B, int nq, int nkv, int num_slots, int max_ctx,
                                       void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!part || !q_out || !k8 || !v8 || !ks || !vs || !cos_t || !sin_t || ks_chunks < 1) return fail(TRACE_ERR_ARG, "null argument");
    TRY(op_attn_decode_state(B, nq, nkv, max_ctx, 1));
    TRY(op_check_slots_pos(slots, pos, B, num_slots, max_ctx, s));
    LCHK(launch_qkv_finish_kv8(part, ks_chunks, (nq + 2 * nkv) * 128, (bf16_t*)q_out, op_kv8(k8, v8, ks, vs, nkv, max_ctx), slots, pos, B, nq, nkv, cos_t,
                               sin_t, s));
    return TRACE_OK;
}
extern "C" int trace_op_kv8_pack(const void* k_rows, const void* v_rows, void* k8, void* v8, float* ks, float* vs, const int32_t* slots, int pos0, int R,
                                 int B, int nkv, int num_slots, int max_ctx, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!k_rows || !v_rows || !k8 || !v8 || !ks || !vs) return fail(TRACE_ERR_ARG, "null argument");
    if (B < 1 || B > SK_ROWS) return fail(TRACE_ERR_ARG, "bad batch (at most " + std::to_string(SK_ROWS) + " rows)");
    if (nkv < 1 || nkv > OP_ATTN_MAX_KV || max_ctx < 32 || max_ctx % 32) return fail(TRACE_ERR_ARG, "bad kv8 cache shape");
    if (R < 1 || pos0 < 0 || (long)pos0 + R > max_ctx) return fail(TRACE_ERR_ARG, "rows outside the slot");
    TRY(op_check_slots(slots, B, num_slots, s));
    LCHK(launch_kv8_pack((const bf16_t*)k_rows, (long)nkv * R * 128, (long)R * 128, 128, (const bf16_t*)v_rows, (long)nkv * R * 128, (long)R * 128, 128,
                         op_kv8(k8, v8, ks, vs, nkv, max_ctx), slots, pos0, R, B, nkv, s));
    return TRACE_OK;
}
extern "C" int trace_op_kv8_unpack(const void* k8, const void* v8, const float* ks, const float* vs, const int32_t* slots, void* k_out, void* vt_out,
                                   int R, int B, int nkv, int num_slots, int max_ctx, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!k8 || !v8 || !ks || !vs || !k_out || !vt_out) return fail(TRACE_ERR_ARG, "null argument");
    if (B < 1 || B > SK_ROWS) return fail(TRACE_ERR_ARG, "bad batch (at most " + std::to_string(SK_ROWS) + " rows)");
    if (nkv < 1 || nkv > OP_ATTN_MAX_KV || max_ctx < 32 || max_ctx % 32) return fail(TRACE_ERR_ARG, "bad kv8 cache shape");
    if (R < 1 || R > max_ctx) return fail(TRACE_ERR_ARG, "rows outside the slot");
    TRY(op_check_slots(slots, B, num_slots, s));
    LCHK(launch_kv8_unpack(op_kv8((void*)k8, (void*)v8, (float*)ks, (float*)vs, nkv, max_ctx), slots, (bf16_t*)k_out, (bf16_t*)vt_out,
                           (long)nkv * max_ctx * 128, (long)max_ctx * 128, max_ctx, R, B, nkv, s));
    return TRACE_OK;
}

// ---- prefill cache-write hooks (llm.hip rope_kv / gather_rows, attn.hip transpose_v; tests/test_gpu_prefill_glue_probes.py) ----
// Thin pass-throughs of the three launchers: every stride and offset is the caller's.  Each takes the ELEMENT COUNT of every array the launch touches and
// answers TRACE_ERR_ARG, before any launch, when a read or a store would leave one of them.
static bool op_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static int op_read_i32(const int32_t* dev, long n, std::vector<int32_t>& host, hipStream_t s) {
    host.resize((size_t)n);
    HIPCHK(hipMemcpyAsync(host.data(), dev, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return TRACE_OK;
}
extern "C" int trace_op_rope_kv(void* qkv, int64_t qkv_elems, int ld, void* kcache, int64_t kcache_elems, void* vcache, int64_t vcache_elems,
                                int64_t slot_stride, int64_t kv_head_stride, const int32_t* slot_arr, const int32_t* pos_arr, int64_t arr_len, int slot0, int pos0,
                                int R, int nq, int nkv, int hd, const float* cos_t, const float* sin_t, int table_rows, int seq_len, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!qkv || !kcache || !cos_t || !sin_t) return fail(TRACE_ERR_ARG, "null argument");
    if (R < 1 || nq < 1 || nkv < 1 || hd < 16 || hd % 16 || seq_len < 0 || table_rows < 1) return fail(TRACE_ERR_ARG, "bad R / heads / hd / seq_len / table_rows");
    const long width = (long)(nq + 2 * nkv) * hd;
    if (ld % 8 || ld < width) return fail(TRACE_ERR_ARG, "ld: a multiple of 8, at least (nq + 2 nkv) hd");
    if (qkv_elems < (long)(R - 1) * ld + width) return fail(TRACE_ERR_ARG, "qkv holds fewer than R rows");
    if (slot_stride < 0 || kv_head_stride < 0 || slot_stride % 8 || kv_head_stride % 8) return fail(TRACE_ERR_ARG, "cache strides: non-negative multiples of 8 elements");
    if (!op_aligned16(qkv) || !op_aligned16(kcache) || !op_aligned16(vcache) || !op_aligned16(cos_t) || !op_aligned16(sin_t))
        return fail(TRACE_ERR_ARG, "pointers must be 16-byte aligned");
    if ((slot_arr || pos_arr) && arr_len < R) return fail(TRACE_ERR_ARG, "slot_arr / pos_arr hold fewer than R entries");
    std::vector<int32_t> hs, hp;
    if (slot_arr) TRY(op_read_i32(slot_arr, R, hs, s));
    if (pos_arr) TRY(op_read_i32(pos_arr, R, hp, s));
    std::vector<int64_t> seen;
    seen.reserve((size_t)R);
    for (int r = 0; r < R; ++r) {                       // the kernel's own rule for a row's slot and position
        const int sq = seq_len > 0 ? r / seq_len : 0;
        const long pos = pos_arr ? (long)hp[r] : (long)pos0 + r - (long)sq * seq_len;
        const long slot = slot_arr ? (long)hs[r] : (long)slot0 + sq;
        if (pos < 0 || pos >= table_rows) return fail(TRACE_ERR_ARG, "position outside the RoPE tables");
        if (slot < 0) return fail(TRACE_ERR_ARG, "slot out of range");
        if ((pos + 1) * hd > kv_head_stride && nkv > 1) return fail(TRACE_ERR_ARG, "position past the kv head's rows");
        const long end = slot * slot_stride + (long)(nkv - 1) * kv_head_stride + (pos + 1) * hd;
        if (end > kcache_elems) return fail(TRACE_ERR_ARG, "slot / position past the K cache");
        if (vcache && end > vcache_elems) return fail(TRACE_ERR_ARG, "slot / position past the V cache");
        seen.push_back(slot * slot_stride + pos * hd);
    }
    if ((long)nkv * kv_head_stride > slot_stride && (slot_arr || (seq_len > 0 && R > seq_len))) return fail(TRACE_ERR_ARG, "kv heads overlap the next slot");
    std::sort(seen.begin(), seen.end());
    for (size_t i = 1; i < seen.size(); ++i)
        if (seen[i] - seen[i - 1] < hd) return fail(TRACE_ERR_ARG, "two rows go to one cache row");
    LCHK(launch_rope_kv((bf16_t*)qkv, ld, (bf16_t*)kcache, (bf16_t*)vcache, (long)slot_stride, (long)kv_head_stride, slot_arr, pos_arr, slot0, pos0, R, nq, nkv,
                        hd, cos_t, sin_t, seq_len, s));
    return TRACE_OK;
}
extern "C" int trace_op_transpose_v(const void* src, int64_t src_elems, int64_t src_bs, int64_t src_hs, int src_rs, void* dst, int64_t dst_elems, int64_t dst_bs,
                                    int64_t dst_hs, int dst_rs, int n, int hd, int heads, int batch, int perm, int p0, void* stream) {
    if (!src || !dst) return fail(TRACE_ERR_ARG, "null argument");
    if (hd != 64 && hd != 128) return fail(TRACE_ERR_ARG, "hd must be 64 or 128");
    if (perm != 0 && perm != 1) return fail(TRACE_ERR_ARG, "perm: 0 or 1");
    if (perm && p0) return fail(TRACE_ERR_ARG, "perm = 1 takes p0 = 0 only");
    if (n < 1 || p0 < 0 || heads < 1 || heads > 65535 || batch < 1 || batch > 65535) return fail(TRACE_ERR_ARG, "bad n / p0 / heads / batch");
    if (dst_rs < 64 || dst_rs % 64 || (long)p0 + n > dst_rs) return fail(TRACE_ERR_ARG, "dst_rs: a multiple of 64, at least p0 + n");
    if (src_rs < hd || src_rs % 8 || src_hs < 0 || src_hs % 8 || src_bs < 0 || src_bs % 8) return fail(TRACE_ERR_ARG, "source strides: multiples of 8, src_rs >= hd");
    if (dst_hs < 0 || dst_hs % 8 || dst_bs < 0 || dst_bs % 8) return fail(TRACE_ERR_ARG, "destination strides: non-negative multiples of 8");
    if (!op_aligned16(src) || !op_aligned16(dst)) return fail(TRACE_ERR_ARG, "pointers must be 16-byte aligned");
    if (src_elems < (long)(batch - 1) * src_bs + (long)(heads - 1) * src_hs + (long)(n - 1) * src_rs + hd) return fail(TRACE_ERR_ARG, "the source holds fewer than n rows");
    const long last = round_up(p0 + n, 64);             // stores end with the zero fill of the last 64-position block
    if (dst_elems < (long)(batch - 1) * dst_bs + (long)(heads - 1) * dst_hs + (long)(hd - 1) * dst_rs + last) return fail(TRACE_ERR_ARG, "the destination is too small");
    LCHK(launch_transpose_v((const bf16_t*)src, (long)src_bs, (long)src_hs, src_rs, (bf16_t*)dst, (long)dst_bs, (long)dst_hs, dst_rs, n, hd, heads, batch,
                            (hipStream_t)stream, perm, p0));
    return TRACE_OK;
}
extern "C" int trace_op_gather_rows(const void* const* tabs, const int64_t* tab_rows, const int32_t* kind, int64_t kind_len, const int32_t* row, int64_t row_len,
                                    void* out, int64_t out_elems, int L, int H, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!tabs || !tab_rows || !kind || !row || !out) return fail(TRACE_ERR_ARG, "null argument");
    if (L < 1 || H < 8 || H % 8) return fail(TRACE_ERR_ARG, "bad L / H (H a multiple of 8)");
    if (kind_len < L || row_len < L) return fail(TRACE_ERR_ARG, "kind / row hold fewer than L entries");
    if (out_elems < (long)L * H) return fail(TRACE_ERR_ARG, "out holds fewer than L rows");
    if (!op_aligned16(out)) return fail(TRACE_ERR_ARG, "pointers must be 16-byte aligned");
    GatherTabs t{};
    for (int k = 0; k < 6; ++k) {
        if (!op_aligned16(tabs[k]) || tab_rows[k] < 0 || (!tabs[k] && tab_rows[k])) return fail(TRACE_ERR_ARG, "bad table");
        t.t[k] = (const bf16_t*)tabs[k];
    }
    std::vector<int32_t> hk, hr;
    TRY(op_read_i32(kind, L, hk, s));
    TRY(op_read_i32(row, L, hr, s));
    for (int r = 0; r < L; ++r) {
        if (hk[r] < 0 || hk[r] > 5) return fail(TRACE_ERR_ARG, "kind outside 0..5");
        if (hr[r] < 0 || hr[r] >= tab_rows[hk[r]]) return fail(TRACE_ERR_ARG, "row outside its table");
    }
    LCHK(launch_gather_rows(t, kind, row, (bf16_t*)out, L, H, s));
    return TRACE_OK;
}
