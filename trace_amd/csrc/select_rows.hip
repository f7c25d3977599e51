// The per-row form of the token selection (select.h, SELECT_PER_ROW): row b samples under its own st.row_sp[b] or takes the arg-max over its head
// range, and keeps its own st.row_max_new[b] in every max_new guard — the selection of a decode batch begun with trace_decode_set_row_params.  Its
// two instantiations (without and with the stop match) live here, so that select.hip and constrain.hip hold the three batch-wide forms each, as before.
#include "select.h"

int launch_select_rows(const float* logits, const StepState& st, const bf16_t* embed, const bf16_t* time_tab, const bf16_t* score_tab, const bf16_t* sync_row,
                       bf16_t* xnext, int ldx, int B, int H, int V, int Tv, int Sv, int advance, hipStream_t s, const ConstrainTable* stop) {
    if (B < 1 || B > SK_ROWS || H % 8 || !logits || !st.row_sp || !st.row_max_new) return TRACE_ERR_ARG;
    const int ntiles = (V + 1 + Tv + Sv + 15) / 16;
    const dim3 grid(B), block(256);
    if (stop)
        hipLaunchKernelGGL((select_next_kernel<SELECT_PER_ROW, true>), grid, block, 0, s, nullptr, nullptr, st, embed, time_tab, score_tab, sync_row, xnext, ldx, B, H,
                           V, Tv, Sv, ntiles, advance, logits, nullptr, stop);
    else
        hipLaunchKernelGGL((select_next_kernel<SELECT_PER_ROW, false>), grid, block, 0, s, nullptr, nullptr, st, embed, time_tab, score_tab, sync_row, xnext, ldx, B, H,
                           V, Tv, Sv, ntiles, advance, logits, nullptr, nullptr);
    return hipGetLastError() == hipSuccess ? TRACE_OK : TRACE_ERR_HIP;
}
