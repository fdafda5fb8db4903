// K50: the match readout with an additive per-key term — the BIAS instantiations of the kernel template in corr_topk_kernel.h
// (K = 1, 2, 4, 8; no labels, no column side).  z_ij = inv_temperature <q_i, k_j> + k_bias[b, j]; per query the k largest z, their
// keys and log sum_j exp z_ij.  One launch of this entry is one half-step of a log-domain Sinkhorn iteration (the bias is the other
// side's potential), and its top-k over z selects the candidates of the transport plan's rows.
#include "corr_topk_kernel.h"

extern "C" int cocos_corr_topk_bias_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, const float* k_bias, int* idx_out,
                                          float* val_out, float* lse_out, int B, int K, int Nq, int Nk, int k, float inv_temperature,
                                          float operand_scale, long long k_batch_stride, cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(k_bias, COCOS_ERR_INVALID, "corr_topk_bias_f16x3: null bias pointer");
    if (const int rc = check_corr_readout("corr_topk_bias_f16x3", "a host-side add to materialised logits and cocos_row_topk_lse", qh, ql, kh,
                                          kl, idx_out, val_out, lse_out, B, K, Nq, Nk, k, inv_temperature, operand_scale, k_batch_stride))
        return rc;
    COCOS_REQUIRE((reinterpret_cast<uintptr_t>(k_bias) & 3) == 0, COCOS_ERR_INVALID, "corr_topk_bias_f16x3: the bias must be 4-byte aligned");
    if (k == 1)
        return launch_corr_topk<1, false, false, true>(qh, ql, kh, kl, idx_out, val_out, lse_out, B, Nq, Nk, k, inv_temperature, operand_scale,
                                                       k_batch_stride, stream, nullptr, nullptr, nullptr, k_bias);
    if (k == 2)
        return launch_corr_topk<2, false, false, true>(qh, ql, kh, kl, idx_out, val_out, lse_out, B, Nq, Nk, k, inv_temperature, operand_scale,
                                                       k_batch_stride, stream, nullptr, nullptr, nullptr, k_bias);
    if (k <= 4)
        return launch_corr_topk<4, false, false, true>(qh, ql, kh, kl, idx_out, val_out, lse_out, B, Nq, Nk, k, inv_temperature, operand_scale,
                                                       k_batch_stride, stream, nullptr, nullptr, nullptr, k_bias);
    return launch_corr_topk<8, false, false, true>(qh, ql, kh, kl, idx_out, val_out, lse_out, B, Nq, Nk, k, inv_temperature, operand_scale,
                                                   k_batch_stride, stream, nullptr, nullptr, nullptr, k_bias);
}
