// The process-wide A/B switches of the kernel launchers as one struct of named values (host only: nothing here reaches device code).  engine.hip holds
// the table that names each field (TUNE_ROWS: dotted name, range, default, what it does), the legacy numeric codes of trace_op_set_gemm_variant
// (LEGACY_CODES) and the C ABI (trace_op_tuning_set / _get / _reset / _name).  Launchers read g_tune and never write it; the setters are for tests and
// tools: not while launches are in flight (the pipeline's two launch threads read these words without a lock).
#pragma once

struct Tuning {
    int gemm_kernel, gemm_w4, gemm_resid_pers, gemm_pers_walk, gemm_pers_opt, gemm_pers_grid_cap, gemm_ldr_opt, gemm_w4_opt;      // gemm*.hip
    int decode_wide_min_rows, decode_wide_fuse_qkv, decode_gemm_tiled, decode_fuse_norm_rows, decode_fuse_swiglu, decode_unfused_qkv;   // engine.hip decode_step*
    int decode_partial_cfg, decode_partial_wgs;                                                                                   // gemm.hip partial-row GEMM
    int attn_decode_debug, attn_decode_waves, attn_decode_nt, attn_decode_lds_pad_kb, attn_decode_nsplit;                         // decode.hip, engine.hip
    int attn_prefill_debug, attn_vit_big, skinny_debug, prefill_last_rows, vit_patch_fused;                                       // attn.hip, decode.hip, engine.hip
};
extern Tuning g_tune;
const Tuning& tuning_initial();      // every field at its default; TRACE_GEMM_W4 / TRACE_PARTIAL_WGS from the environment, read once
