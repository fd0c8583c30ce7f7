// train_exec.hip -- the train-mode MinkUNet body forward and backward behind ONE C call each (include/pbnet_hip.h:
// pbn_unet_train_forward / _backward).  Only sequences the kernels of spconv.hip / spconv_wave.hip (convolutions and
// their input gradients), bnorm.hip (batch norm with the block tail) and wgrad.hip; no new arithmetic lives here.
// Mirrors /root/reference/network/Mink.py:291-350 in training mode (MinkowskiEngine's BasicBlock.forward for the stages).
#include "spconv_common.h"
#include "unet_plan.h"

using namespace pbn;

namespace {

inline bool op_ok(const pbn_train_op& o, int n_bufs) {
    return op_index_ok(o.in_buf, o.res_buf, o.out_buf, o.level_in, o.level_out, n_bufs) && o.pre_buf >= 1 && o.pre_buf < n_bufs &&
           o.gamma && o.beta && o.cout == o.cout_p && o.w;
}

// both tables of an op: the backward needs the one of the input gradient as well
inline OpTables train_tables(const pbn_train_op& o, const MapTables& t) {
    OpTables m = op_tables(o.map_kind, o.level_in, o.level_out, t);
    m.ok = m.ok && (o.map_kind == 0 || m.bwd != nullptr);
    return m;
}

}  // namespace

extern "C" int pbn_unet_train_forward(const pbn_train_op* ops, int n_ops, const pbn_unet_buf* bufs, int n_bufs,
                                      const int32_t* n_rows, const void* input, int ld_input, const int32_t* const* k3,
                                      const int32_t* k5, const int32_t* const* down, const int32_t* const* up, void* act_arena,
                                      size_t arena_bytes, float* stats, int dtype, void* splitk_ws, size_t splitk_bytes,
                                      void* bn_ws, size_t bn_ws_bytes, pbn_stream_t stream) {
    if (!ops || !bufs || !n_rows || !input || !act_arena || !stats || n_ops < 1 || n_bufs < 2 || n_bufs > 512) return PBN_ERR_ARG;
    int64_t offs[512];
    if (pbn_unet_arena_bytes(bufs, n_bufs, n_rows, dtype, offs) > arena_bytes) return PBN_ERR_WORKSPACE;
    const PlanArena X(act_arena, offs, bufs, input, ld_input, esize(dtype));
    const MapTables T{k3, k5, down, up};
    for (int i = 0; i < n_ops; ++i) {
        const pbn_train_op& o = ops[i];
        if (!op_ok(o, n_bufs)) return PBN_ERR_ARG;
        const OpTables m = train_tables(o, T);
        if (!m.ok) return PBN_ERR_ARG;
        const int n_in = n_rows[o.level_in], n_out = n_rows[o.level_out];
        void* pre = X.at(o.pre_buf);
        int rc = spconv_launch({.in_feat = X.at(o.in_buf, o.in_col), .ld_in = X.ld(o.in_buf), .n_in = n_in, .nbr = m.fwd,
                                .n_offsets = m.K, .n_out = n_out, .w_packed = o.w, .vecs_per_offset = o.vpo, .n_steps = o.n_steps,
                                .cout_padded = o.cout_p, .out_feat = pre, .ld_out = X.ld(o.pre_buf), .dtype = dtype,
                                .workspace = splitk_ws, .workspace_bytes = splitk_bytes},
                               ConvHints{}, (hipStream_t)stream);
        if (rc != PBN_OK) return rc;
        const void* res = o.res_buf >= 0 ? X.at(o.res_buf, o.res_col) : nullptr;
        rc = pbn_bn_act_train_forward(pre, X.ld(o.pre_buf), n_out, o.cout, dtype, o.gamma, o.beta, o.eps, o.momentum,
                                      o.running_mean, o.running_var, res, o.res_buf >= 0 ? X.ld(o.res_buf) : 0, o.relu,
                                      X.at(o.out_buf, o.out_col), X.ld(o.out_buf), stats + o.stat_off,
                                      stats + o.stat_off + o.cout, bn_ws, bn_ws_bytes, stream);
        if (rc != PBN_OK) return rc;
    }
    return PBN_OK;
}

extern "C" int pbn_unet_train_backward(const pbn_train_op* ops, int n_ops, const pbn_unet_buf* bufs, int n_bufs,
                                       const int32_t* n_rows, const void* input, int ld_input, const int32_t* const* k3,
                                       const int32_t* k5, const int32_t* const* down, const int32_t* const* up,
                                       const pbn_pair_lists* pairs, const void* act_arena, void* grad_arena, size_t arena_bytes,
                                       const float* stats, float* param_grads, void* dinput, int ld_dinput, int dtype,
                                       void* splitk_ws, size_t splitk_bytes, void* bn_ws, size_t bn_ws_bytes, void* wgrad_ws,
                                       size_t wgrad_ws_bytes, pbn_stream_t stream) {
    if (!ops || !bufs || !n_rows || !input || !pairs || !act_arena || !grad_arena || !stats || !param_grads || n_ops < 1 ||
        n_bufs < 2 || n_bufs > 512)
        return PBN_ERR_ARG;
    int64_t offs[512];
    if (pbn_unet_arena_bytes(bufs, n_bufs, n_rows, dtype, offs) > arena_bytes) return PBN_ERR_WORKSPACE;
    const int es = esize(dtype);
    const PlanArena X(act_arena, offs, bufs, input, ld_input, es);        // activations of the forward
    const PlanArena G(grad_arena, offs, bufs, dinput, ld_dinput, es);     // their gradients, the same layout
    const MapTables T{k3, k5, down, up};
    for (int i = n_ops - 1; i >= 0; --i) {
        const pbn_train_op& o = ops[i];
        if (!op_ok(o, n_bufs)) return PBN_ERR_ARG;
        const OpTables m = train_tables(o, T);
        if (!m.ok) return PBN_ERR_ARG;
        const int n_in = n_rows[o.level_in], n_out = n_rows[o.level_out];
        // 1. batch norm with its tail: g = d(pre), the masked gradient to the residual branch
        char* gpre = G.at(o.pre_buf);
        const char* y = X.at(o.out_buf, o.out_col);
        if (o.res_buf >= 0 && !o.relu) return PBN_ERR_UNSUPPORTED;      // the residual gradient is then dy itself: not on the path
        int rc = pbn_bn_act_train_backward(X.at(o.pre_buf), X.ld(o.pre_buf), G.at(o.out_buf, o.out_col), G.ld(o.out_buf),
                                           o.relu ? y : nullptr, o.relu ? X.ld(o.out_buf) : 0, n_out, o.cout, dtype, o.gamma,
                                           stats + o.stat_off, stats + o.stat_off + o.cout, gpre, G.ld(o.pre_buf),
                                           o.res_buf >= 0 ? G.at(o.res_buf, o.res_col) : nullptr,
                                           o.res_buf >= 0 ? G.ld(o.res_buf) : 0, param_grads + o.dgamma_off,
                                           param_grads + o.dbeta_off, bn_ws, bn_ws_bytes, stream);
        if (rc != PBN_OK) return rc;
        // 2. input gradient on the convolution kernel (the mirrored / up / down table), accumulated in the epilogue
        if (o.want_dx) {
            if (!o.w_d || (o.in_buf == 0 && !dinput)) return PBN_ERR_ARG;
            char* dx = G.at(o.in_buf, o.in_col);
            rc = spconv_launch({.in_feat = gpre, .ld_in = G.ld(o.pre_buf), .n_in = n_out, .nbr = m.bwd, .n_offsets = m.K, .n_out = n_in,
                                .w_packed = o.w_d, .vecs_per_offset = o.vpo_d, .n_steps = o.n_steps_d, .cout_padded = o.cout_p_d,
                                .residual = o.dx_accumulate ? dx : nullptr, .ld_res = o.dx_accumulate ? G.ld(o.in_buf) : 0,
                                .out_feat = dx, .ld_out = G.ld(o.in_buf), .dtype = dtype, .workspace = splitk_ws,
                                .workspace_bytes = splitk_bytes},
                               ConvHints{}, (hipStream_t)stream);
            if (rc != PBN_OK) return rc;
        }
        // 3. weight gradient over the rule pairs of the forward map
        const void* x = X.at(o.in_buf, o.in_col);
        if (o.map_kind == 0) {
            rc = pbn_spconv_wgrad_checked(x, X.ld(o.in_buf), n_in, gpre, G.ld(o.pre_buf), n_out, dtype, nullptr, nullptr, nullptr,
                                          nullptr, 0, 0, n_out, 1, o.cin, o.cout, param_grads + o.dw_off, wgrad_ws, wgrad_ws_bytes,
                                          stream);
        } else {
            const pbn_pair_lists& P = pairs[m.pair_slot];
            if (!P.in_idx || !P.out_idx || !P.seg_begin) return PBN_ERR_ARG;
            rc = pbn_spconv_wgrad_checked(x, X.ld(o.in_buf), n_in, gpre, G.ld(o.pre_buf), n_out, dtype, P.in_idx, P.out_idx,
                                          P.seg_begin, P.counts, 0, P.segment, P.n_pairs_estimate, m.K, o.cin, o.cout,
                                          param_grads + o.dw_off, wgrad_ws, wgrad_ws_bytes, stream);
        }
        if (rc != PBN_OK) return rc;
    }
    return PBN_OK;
}
