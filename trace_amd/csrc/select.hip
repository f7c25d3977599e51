// The token selection of a decode step: select_next_kernel, one workgroup per sequence, and its one launcher.  Four forms: the arg-max over the
// tile partials of head_logits_kernel (greedy), the sampler (sample.h) over a row of masked logits, the arg-max over a processed logits row
// (the step with logits processors, logits.h), and the per-row form that picks one of the last two by the row's own params (select_rows.hip).  Forced ids, EOS, record_feed, the head switch and the embedding gather are one body (select.h);
// the forms that also match stop sequences are constrain.hip's.
#include "select.h"

int launch_select(int form, const float* part_val, const int32_t* part_idx, const float* logits, const SampleParams* sp, const StepState& st,
                  const bf16_t* embed, const bf16_t* time_tab, const bf16_t* score_tab, const bf16_t* sync_row, bf16_t* xnext, int ldx, int B, int H,
                  int V, int Tv, int Sv, int advance, hipStream_t s, const ConstrainTable* stop) {
    if (B < 1 || B > SK_ROWS || H % 8) return TRACE_ERR_ARG;
    if ((form != SELECT_TILES) != (logits != nullptr) || (form == SELECT_SAMPLE) != (sp != nullptr)) return TRACE_ERR_ARG;
    if (form == SELECT_PER_ROW) return launch_select_rows(logits, st, embed, time_tab, score_tab, sync_row, xnext, ldx, B, H, V, Tv, Sv, advance, s, stop);
    if (stop) return launch_select_stop(form, part_val, part_idx, logits, sp, st, embed, time_tab, score_tab, sync_row, xnext, ldx, B, H, V, Tv, Sv, advance, s, stop);
    return launch_select_forms<false>(form, part_val, part_idx, logits, sp, st, embed, time_tab, score_tab, sync_row, xnext, ldx, B, H, V, Tv, Sv, advance, s, nullptr);
}
