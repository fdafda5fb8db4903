// K36a / K39a / K47: the entry points of the match readout of the split-precision correlation — per query the k largest logits, their
// key indices and the row log-sum-exp.  The kernel template, its launcher and the argument checks live in corr_topk_kernel.h (shared
// with corr_match_mutual_f16x3.hip); this translation unit instantiates K = 1, 2, 4, 8 with and without labels.
#include "corr_topk_kernel.h"

extern "C" int cocos_corr_topk_max_k(void) { return cocos::CT_MAX_K; }

// idx_out / max_out [B,Nq] is the same memory as the [B,Nq,1] of the K = 1 instantiation
extern "C" int cocos_corr_match_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, int* idx_out,
                                      float* max_out, float* lse_out, int B, int K, int Nq, int Nk, float inv_temperature,
                                      float operand_scale, long long k_batch_stride, cocos_stream_t stream) {
    using namespace cocos;
    if (const int rc = check_corr_readout("corr_match_f16x3", "cocos_row_argmax_lse", qh, ql, kh, kl, idx_out, max_out, lse_out, B, K, Nq,
                                          Nk, 1, inv_temperature, operand_scale, k_batch_stride))
        return rc;
    return launch_corr_topk<1>(qh, ql, kh, kl, idx_out, max_out, lse_out, B, Nq, Nk, 1, inv_temperature, operand_scale, k_batch_stride, stream);
}

extern "C" int cocos_corr_topk_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, int* idx_out, float* val_out,
                                     float* lse_out, int B, int K, int Nq, int Nk, int k, float inv_temperature,
                                     float operand_scale, long long k_batch_stride, cocos_stream_t stream) {
    using namespace cocos;
    if (const int rc = check_corr_readout("corr_topk_f16x3", "cocos_row_topk_lse", qh, ql, kh, kl, idx_out, val_out, lse_out, B, K, Nq, Nk,
                                          k, inv_temperature, operand_scale, k_batch_stride))
        return rc;
    if (k == 1)
        return launch_corr_topk<1>(qh, ql, kh, kl, idx_out, val_out, lse_out, B, Nq, Nk, k, inv_temperature, operand_scale, k_batch_stride, stream);
    if (k == 2)
        return launch_corr_topk<2>(qh, ql, kh, kl, idx_out, val_out, lse_out, B, Nq, Nk, k, inv_temperature, operand_scale, k_batch_stride, stream);
    if (k <= 4)
        return launch_corr_topk<4>(qh, ql, kh, kl, idx_out, val_out, lse_out, B, Nq, Nk, k, inv_temperature, operand_scale, k_batch_stride, stream);
    return launch_corr_topk<8>(qh, ql, kh, kl, idx_out, val_out, lse_out, B, Nq, Nk, k, inv_temperature, operand_scale, k_batch_stride, stream);
}

// K47: the same readout over the keys each query's label allows
extern "C" int cocos_corr_topk_labels_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, const int* q_label,
                                            const int* k_label, int* idx_out, float* val_out, float* lse_out, int B, int K, int Nq,
                                            int Nk, int k, float inv_temperature, float operand_scale, long long k_batch_stride,
                                            cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(q_label && k_label, COCOS_ERR_INVALID, "corr_topk_labels_f16x3: null label pointer");
    if (const int rc = check_corr_readout("corr_topk_labels_f16x3", "a host-side mask of materialised logits and cocos_row_topk_lse", qh, ql,
                                          kh, kl, idx_out, val_out, lse_out, B, K, Nq, Nk, k, inv_temperature, operand_scale, k_batch_stride))
        return rc;
    COCOS_REQUIRE((reinterpret_cast<uintptr_t>(q_label) & 3) == 0 && (reinterpret_cast<uintptr_t>(k_label) & 3) == 0, COCOS_ERR_INVALID,
                  "corr_topk_labels_f16x3: label arrays must be 4-byte aligned");
    if (k == 1)
        return launch_corr_topk<1, true>(qh, ql, kh, kl, idx_out, val_out, lse_out, B, Nq, Nk, k, inv_temperature, operand_scale,
                                         k_batch_stride, stream, q_label, k_label);
    if (k == 2)
        return launch_corr_topk<2, true>(qh, ql, kh, kl, idx_out, val_out, lse_out, B, Nq, Nk, k, inv_temperature, operand_scale,
                                         k_batch_stride, stream, q_label, k_label);
    if (k <= 4)
        return launch_corr_topk<4, true>(qh, ql, kh, kl, idx_out, val_out, lse_out, B, Nq, Nk, k, inv_temperature, operand_scale,
                                         k_batch_stride, stream, q_label, k_label);
    return launch_corr_topk<8, true>(qh, ql, kh, kl, idx_out, val_out, lse_out, B, Nq, Nk, k, inv_temperature, operand_scale,
                                     k_batch_stride, stream, q_label, k_label);
}
