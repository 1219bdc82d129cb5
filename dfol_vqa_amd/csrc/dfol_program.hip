// The native executor of a lowered ProgramBatch: ONE C-ABI call enqueues every launch of a batch's forward (scene stage + operators).
//
// The reference runs one Python dispatch per operator (batch_base_interpreter.py:145-172 -> batch_gqa_interpreter.py:72-78 -> the operator
// classes of batch_gqa_ops.py), each of which issues a few tensor ops; at MI355X speed the ~35 launches of a fresh 256-question batch
// cost ~55 us of Python each while their kernels take 1.7 - 2.1 ms together (profiles/r04: the device idles for half of the step).
// Here the host lowers a collated ProgramBatch ONCE, in the collate worker, to a table of kernel-level instructions
// (dfol_vqa_amd/native_plan.py) and this function walks the table, calling the very same entry points of this library the Python
// operators call - same kernels, same arguments, so the results are bit-identical to the Python loop's (tests/test_native_gpu.py).
//
// Memory: `blob` holds every small side array of the batch (geometry, columns, negation / validity flags, predicate -> question maps,
// segment offsets, quantifiers, gate flags, pair-kernel requests), uploaded by the caller with ONE copy; `workspace` is one caller-owned
// arena in which the plan has assigned every intermediate (object matrix, hidden activations, likelihood blocks, relation tiles,
// attentions) and, at its start, the results the host reads back (log-probabilities, arg-max flags).  No allocation, no synchronisation,
// no global state: the call only enqueues work on `stream`, and everything it reads is in its arguments - the feature source in the scene
// struct (DFOL_FEATURES_*), the gate table in the model struct.  The one thread-local the kernels it launches see is the fp16-range status
// word (dfol_set_range_status, dfol_logic.hip), which every entry point of the library reads, not the executor alone.
#include <string.h>

#include "dfol_calib.h"
#include "dfol_common.h"

namespace {

// ---- a run of the attention-calibration passes in ONE launch (DFOL_OP_CALIB_WALK) -----------------------------------------------------------------
// The passes (batch_base_interpreter.py:87-140) are a chain of small row-wise steps over [rows, 50] LSTM states - a cell, a gate between two states, a
// sum, the attention-output product - each of which reads what the step before wrote: eight cells and about as many small steps per forward, ~9 us per
// cell launch and ~5 - 7 us per small one with the device otherwise idle.  Every step treats the rows independently, so a workgroup that owns
// LC_ROWS rows can run the whole chain on them with workgroup barriers between the steps (a workgroup's own global writes are visible to it after a
// barrier: its wavefronts share the CU's L1).  The steps come as a table of WALK_* entries in the blob; they call the same device functions as the
// stand-alone kernels (dfol_calib.h), so the results are bit-identical to the launches they replace.
__global__ __launch_bounds__(LC_THREADS) void calib_walk_kernel(const int64_t* __restrict__ table, int n_steps, int rows, char* __restrict__ ws,
                                                                const char* __restrict__ blob, DfolProgramModel m) {
    extern __shared__ __attribute__((aligned(16))) float cw_s[];
    const int r0 = blockIdx.x * LC_ROWS, tid = threadIdx.x;
    auto W = [&](int64_t off) { return off < 0 ? nullptr : reinterpret_cast<float*>(ws + off); };
    for (int i = 0; i < n_steps; ++i) {
        const int64_t* a = table + (int64_t)i * DFOL_INSTR_WIDTH;
        switch (a[0]) {
            case DFOL_WALK_FILL: {       // dst, planes, width, bits
                uint32_t* dst = reinterpret_cast<uint32_t*>(W(a[1]));
                const int planes = (int)a[2], width = (int)a[3];
                for (int e = tid; e < planes * LC_ROWS * width; e += LC_THREADS) {
                    const int pl = e / (LC_ROWS * width), rem = e - pl * LC_ROWS * width, row = r0 + rem / width;
                    if (row < rows) dst[((int64_t)pl * rows + row) * width + rem % width] = (uint32_t)a[4];
                }
                break;
            }
            case DFOL_WALK_SELECT:       // x, y, flags (blob), planes, width, out
            case DFOL_WALK_ADD: {        // x, y, -, planes, width, out
                const float* x = W(a[1]);
                const float* y = W(a[2]);
                const uint8_t* flags = a[0] == DFOL_WALK_SELECT ? reinterpret_cast<const uint8_t*>(blob + a[3]) : nullptr;
                const int planes = (int)a[4], width = (int)a[5];
                float* out = W(a[6]);
                for (int e = tid; e < planes * LC_ROWS * width; e += LC_THREADS) {
                    const int pl = e / (LC_ROWS * width), rem = e - pl * LC_ROWS * width, row = r0 + rem / width;
                    if (row < rows) {
                        const int64_t pr = (int64_t)pl * rows + row, at_ = pr * width + rem % width;
                        out[at_] = flags ? (flags[pr] ? x : y)[at_] : x[at_] + y[at_];
                    }
                }
                break;
            }
            case DFOL_WALK_LSTM: {       // which, h, c, h_out, c_out, head (blob), n_head, table (blob), E, idx (blob)
                const int w = a[1] ? 1 : 0;
                LcCell p{nullptr, 0, m.lstm_kx, W(a[2]), m.lstm_h, W(a[3]), m.lstm_wih_t[w], m.lstm_ld_wih[w], m.lstm_whh_t[w], m.lstm_ld_whh[w], m.lstm_bih[w],
                         m.lstm_bhh[w], rows, m.lstm_h, W(a[4]), W(a[5]), nullptr,
                         LcTokens{reinterpret_cast<const float*>(blob + a[6]), (int)a[7], reinterpret_cast<const float*>(blob + a[8]), (int)a[9],
                                  reinterpret_cast<const int32_t*>(blob + a[10])}};
                lc_stage(p, r0, cw_s);
                __syncthreads();
                lc_wide(p, r0, cw_s, cw_s + LC_ROWS * (m.lstm_kx + m.lstm_h));
                break;
            }
            case DFOL_WALK_ATT_MODULATIONS:  // forward state h, backward state h, out
                if (tid < 256) am_rows(W(a[1]), W(a[2]), m.att_out_w, m.ld_att_out, m.att_out_b, rows, m.lstm_h, m.att_out_n, W(a[3]), r0, tid);
                break;
            default: break;
        }
        __syncthreads();
    }
}

int run_calib_walk(const DfolProgramModel* model, const int64_t* table_dev, int32_t n_steps, int32_t rows, void* workspace, const void* blob, void* stream) {
    DFOL_REQUIRE(n_steps >= 0 && rows >= 0, "calib_walk: bad sizes");
    if (n_steps == 0 || rows == 0) return 0;
    DFOL_REQUIRE(model->lstm_wih_t[0] && model->lstm_whh_t[0] && model->lstm_wih_t[1] && model->lstm_whh_t[1] && model->lstm_h > 0 && model->lstm_kx > 0 &&
                     model->att_out_w && model->att_out_n > 0,
                 "calib_walk: the model has no calibration networks");
    DFOL_REQUIRE(lc_walk_fits(model->lstm_kx, model->lstm_h),
                 "calib_walk: input width %d + hidden %d too large for the staging buffer (KX + 9 H + 2 <= 1024: dfol_calib_walk_supported)", model->lstm_kx,
                 model->lstm_h);
    const size_t lds = sizeof(float) * lc_wide_lds_floats(model->lstm_kx, model->lstm_h);
    hipLaunchKernelGGL(calib_walk_kernel, dim3(dfol_cdiv(rows, LC_ROWS)), dim3(LC_THREADS), lds, (hipStream_t)stream, table_dev, n_steps, rows,
                       static_cast<char*>(workspace), static_cast<const char*>(blob), *model);
    DFOL_LAUNCH_CHECK("calib_walk");
    return 0;
}

inline const void* at(const void* base, int64_t off) { return off < 0 ? nullptr : static_cast<const char*>(base) + off; }
inline void* at(void* base, int64_t off) { return off < 0 ? nullptr : static_cast<char*>(base) + off; }

int run_dense(const DfolDenseLayer& L, const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t M, void* stream) {
    // the dispatch of _lib.linear_act: the split-operand kernels for weights of >= 65536 elements when the input view allows it
    DFOL_REQUIRE(L.kind != DFOL_DENSE_HEAD_F16X2, "run_program: a DFOL_DENSE_HEAD_F16X2 layer runs inside DFOL_OP_ATTR_HEAD, not as a dense product");
    const bool split_ok = L.kind != DFOL_DENSE_F32 && L.packed != nullptr && L.K % 4 == 0 && ldx % 2 == 0 && (reinterpret_cast<uintptr_t>(X) % 8 == 0);
    if (!split_ok) return dfol_linear_act_f32(X, ldx, L.weight, L.ldw, L.bias, Y, ldy, M, L.N, L.K, L.act, stream);
    switch (L.kind) {
        case DFOL_DENSE_F16X2: return dfol_linear_act_h2_f32(X, ldx, L.packed, L.bias, Y, ldy, M, L.N, L.K, L.act, stream);
        case DFOL_DENSE_BF16X3: return dfol_linear_act_split_f32(X, ldx, L.packed, L.bias, Y, ldy, M, L.N, L.K, L.act, stream);
        case DFOL_DENSE_BF16: return dfol_linear_act_bf16_f32(X, ldx, L.packed, L.bias, Y, ldy, M, L.N, L.K, L.act, stream);
    }
    dfol_set_error("run_program: unknown dense kind %d", L.kind);
    return 1;
}

// DFOL_OP_PAIR_LL: the entry points that take a packed image of W2, by DFOL_PAIR_* (DFOL_PAIR_PLAIN reads the weight itself: another argument list)
using PairImageEntry = int (*)(const float*, int64_t, int32_t, const float*, int64_t, const float*, const void*, const float*, int32_t, const float*, int64_t,
                               const float*, const int32_t*, const int32_t*, int32_t, int32_t, const int32_t*, const int32_t*, const uint8_t*, int32_t, int32_t,
                               float, int32_t, void*, void*);
template <class... Rest>       // (the fp32 image alone is declared const float*)
int pair_ll_packed(const float* uv, int64_t ld_uv, int32_t hid1, const float* pos, int64_t ld_pos, const float* wg, const void* w2, Rest... rest) {
    return dfol_pair_ll_packed_f32(uv, ld_uv, hid1, pos, ld_pos, wg, static_cast<const float*>(w2), rest...);
}
constexpr PairImageEntry kPairImageEntry[] = {nullptr, pair_ll_packed, dfol_pair_ll_split_f32, dfol_pair_ll_h2_f32, dfol_pair_ll_h1_f32};
static_assert(DFOL_PAIR_PACKED == 1 && DFOL_PAIR_BF16X3 == 2 && DFOL_PAIR_F16X2 == 3 && DFOL_PAIR_F16 == 4, "kPairImageEntry is indexed by DFOL_PAIR_*");

constexpr const char* kFeatureForm[] = {"DFOL_FEATURES_MATRIX",       "DFOL_FEATURES_ROWS_F32",         "DFOL_FEATURES_ROWS_BF16",
                                         "DFOL_FEATURES_ROWS_BF16_H2", "DFOL_FEATURES_ROWS_BF16_H2_F16", "DFOL_FEATURES_CACHED"};
static_assert(DFOL_FEATURES_MATRIX == 0 && DFOL_FEATURES_ROWS_F32 == 1 && DFOL_FEATURES_ROWS_BF16 == 2 && DFOL_FEATURES_ROWS_BF16_H2 == 3 &&
                  DFOL_FEATURES_ROWS_BF16_H2_F16 == 4 && DFOL_FEATURES_CACHED == 5,
              "kFeatureForm is indexed by DFOL_FEATURES_*");
inline bool rows_form(int32_t form) { return form >= DFOL_FEATURES_ROWS_F32 && form <= DFOL_FEATURES_ROWS_BF16_H2_F16; }

// The source-0 DFOL_OP_DENSE of a scene in one of the index forms: the featurizer's first product reads the store's rows in place, by the
// form's own kernel - the matrix route's bits.  A layer the form does not admit is refused before anything is launched.
int run_first_layer_rows(const DfolProgramScene& sc, const DfolDenseLayer& L, int64_t x_off, float* Y, int64_t ldy, int32_t M, void* stream) {
    const char* form = kFeatureForm[sc.feature_form];
    switch (sc.feature_form) {
        case DFOL_FEATURES_ROWS_F32:         // an fp32 table in front of the default arithmetic
            DFOL_REQUIRE(x_off == 0 && L.kind == DFOL_DENSE_F16X2 && L.packed != nullptr && dfol_linear_wide_supported(M, L.N, L.K),
                         "run_program: a scene in index form (%s) needs a two-piece fp16 product of a shape dfol_linear_wide_supported takes "
                         "(M %d N %d K %d kind %d): hand over the gathered matrix", form, M, L.N, L.K, L.kind);
            return dfol_linear_wide_rows_h2_f32(sc.features, sc.ld_features, sc.src_row, L.packed, L.bias, Y, ldy, M, L.N, L.K, L.act, stream);
        case DFOL_FEATURES_ROWS_BF16:        // a bf16 table: the bf16 mode's product over its rows
            DFOL_REQUIRE(x_off == 0 && L.kind == DFOL_DENSE_BF16 && L.packed != nullptr && dfol_linear_rows_bf16t_supported(L.N, L.K, sc.ld_features),
                         "run_program: a scene in bf16 index form (%s) needs a DFOL_DENSE_BF16 first layer of a shape "
                         "dfol_linear_rows_bf16t_supported takes (N %d K %d ld %lld kind %d): hand over the gathered matrix", form, L.N, L.K,
                         (long long)sc.ld_features, L.kind);
            return dfol_linear_act_rows_bf16t_f32(sc.features, sc.ld_features, sc.src_row, L.packed, L.bias, Y, ldy, M, L.N, L.K, L.act, stream);
        case DFOL_FEATURES_ROWS_BF16_H2:     // a bf16 table in front of the default arithmetic: split in place
        case DFOL_FEATURES_ROWS_BF16_H2_F16: // ... certified to hold fp16 values: two products instead of three
            DFOL_REQUIRE(L.kind == DFOL_DENSE_F16X2,
                         "run_program: a scene in bf16 index form for the two-piece fp16 product (%s) needs a DFOL_DENSE_F16X2 first layer, this one "
                         "is of kind %d: DFOL_FEATURES_ROWS_BF16 serves a DFOL_DENSE_BF16 layer, every other arithmetic takes the gathered matrix", form,
                         L.kind);
            DFOL_REQUIRE(x_off == 0 && L.packed != nullptr && dfol_linear_wide_rows_bf16t_supported(M, L.N, L.K, sc.ld_features),
                         "run_program: a scene in bf16 index form (%s) needs a first layer of a shape dfol_linear_wide_rows_bf16t_supported takes "
                         "(M %d N %d K %d ld %lld): hand over the gathered matrix", form, M, L.N, L.K, (long long)sc.ld_features);
            return dfol_linear_wide_rows_bf16t_f16_h2_f32(sc.features, sc.ld_features, sc.src_row, L.packed, L.bias, Y, ldy, M, L.N, L.K, L.act,
                                                          sc.feature_form == DFOL_FEATURES_ROWS_BF16_H2_F16 ? 1 : 0, stream);
    }
    dfol_set_error("run_program: %s is no index form", form);
    return 1;
}

}  // namespace

extern "C" int dfol_calib_walk_supported(int32_t KX, int32_t H) { return lc_walk_fits(KX, H) ? 1 : 0; }

extern "C" int dfol_run_program(const DfolProgramModel* model, const DfolProgramScene* scene, const int64_t* instr_host, int32_t n_instr,
                                const void* blob, void* workspace, void* stream) {
    DFOL_REQUIRE(model && scene && instr_host && blob && workspace, "run_program: null pointer");
    DFOL_REQUIRE(n_instr >= 0 && scene->NS > 0 && scene->NS % 4 == 0, "run_program: bad sizes (n_instr %d, NS %d)", n_instr, scene->NS);
    const int32_t form = scene->feature_form;
    DFOL_REQUIRE(form >= DFOL_FEATURES_MATRIX && form <= DFOL_FEATURES_CACHED, "run_program: scene->feature_form %d is no DFOL_FEATURES_* form", form);
    DFOL_REQUIRE((scene->src_row != nullptr) == (form != DFOL_FEATURES_MATRIX) && (scene->box6 != nullptr) == (form != DFOL_FEATURES_MATRIX),
                 "run_program: scene->src_row and scene->box6 come together, with every form but DFOL_FEATURES_MATRIX and not with it (%s, src_row %p, box6 %p)",
                 kFeatureForm[form], (const void*)scene->src_row, (const void*)scene->box6);
    DFOL_REQUIRE((scene->cache != nullptr) == (form == DFOL_FEATURES_CACHED), "run_program: scene->cache comes with DFOL_FEATURES_CACHED, and with it alone (%s, cache %p)",
                 kFeatureForm[form], (const void*)scene->cache);
    DFOL_REQUIRE(form != DFOL_FEATURES_CACHED || (scene->cache_cols > 0 && scene->ld_cache >= scene->cache_cols),
                 "run_program: DFOL_FEATURES_CACHED: bad sizes cache_cols=%d ld_cache=%lld", scene->cache_cols, (long long)scene->ld_cache);
    const float* gates = model->gates;
    const int32_t n_gates = model->n_gates;
    DFOL_REQUIRE(n_gates >= 0 && (gates == nullptr) == (n_gates == 0), "run_program: model->gates / model->n_gates: a table of %d gates at %p", n_gates,
                 (const void*)gates);
    // the 18 floats of gate `slot` (+ k: the second axis of an arity-2 cell); the slot was checked by DFOL_GATE_SLOT
    auto gate_row = [&](int64_t slot, int k) { return gates + (slot + k) * 18; };
#define DFOL_GATE_SLOT(slot, arity)                                                                                                                   \
    DFOL_REQUIRE(gates != nullptr && (slot) >= 0 && (slot) + (arity) <= n_gates,                                                                       \
                 "run_program[%d]: opcode %lld names gate slot %lld (arity %d) of a table of %d gates (DfolProgramModel.gates / n_gates)", i,        \
                 (long long)a[0], (long long)(slot), (arity), n_gates)
    const int32_t NS = scene->NS;
    const int32_t* n_obj = static_cast<const int32_t*>(at(blob, scene->n_obj));            // per QUESTION
    const int32_t* img_n_obj = static_cast<const int32_t*>(at(blob, scene->img_n_obj));    // per SCENE (= n_obj without shared scenes)
    const int32_t* obj_off = static_cast<const int32_t*>(at(blob, scene->obj_off));
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int32_t i = 0; i < n_instr; ++i) {
        const int64_t* a = instr_host + static_cast<int64_t>(i) * DFOL_INSTR_WIDTH;
        int rc = 0;
        switch (a[0]) {
            case DFOL_OP_DENSE: {        // set, layer, x source (0 = the raw features, 1 = workspace), x, ldx, y, ldy, M
                const DfolDenseLayer* layers = a[1] == 0 ? model->featurizer : (a[1] == 1 ? model->attribute : &model->uv);
                const int32_t count = a[1] == 0 ? model->n_featurizer : (a[1] == 1 ? model->n_attribute : 1);
                DFOL_REQUIRE(layers && a[2] >= 0 && a[2] < count, "run_program[%d]: dense layer %lld of set %lld does not exist", i, (long long)a[2], (long long)a[1]);
                if (a[1] == 0 && form == DFOL_FEATURES_CACHED) break;    // the featurizer's output comes from the cache (DFOL_OP_BOX_POSITIONS writes it)
                const float* X = a[3] == 0 ? scene->features + a[4] / 4 : static_cast<const float*>(at(workspace, a[4]));
                DfolDenseLayer layer = layers[a[2]];
                if (a[9]) layer.act = DFOL_ACT_NONE;
                if (a[3] == 0 && rows_form(form)) {                 // the scene in index form: the featurizer's first product reads the store's rows
                    rc = run_first_layer_rows(*scene, layer, a[4], static_cast<float*>(at(workspace, a[6])), a[7], static_cast<int32_t>(a[8]), stream);
                    break;
                }
                rc = run_dense(layer, X, a[3] == 0 ? scene->ld_features : a[5], static_cast<float*>(at(workspace, a[6])), a[7], static_cast<int32_t>(a[8]), stream);
                break;
            }
            case DFOL_OP_BOX_POSITIONS:  // obj, ld_obj, pos_col
                if (form == DFOL_FEATURES_CACHED) {                 // (cached form: the object matrix's feature columns and its positions in one launch)
                    DFOL_REQUIRE(a[3] == scene->cache_cols, "run_program[%d]: cached featurizer rows of %d columns (DFOL_FEATURES_CACHED: cache_cols) for an object matrix of %lld + 4",
                                 i, scene->cache_cols, (long long)a[3]);
                    rc = dfol_store_objects_f32(scene->cache, scene->ld_cache, scene->src_row, scene->box6, scene->O, scene->cache_cols,
                                                static_cast<float*>(at(workspace, a[1])), a[2], stream);
                    break;
                }
                if (rows_form(form)) {                              // (index form: the six box columns travel beside the row numbers)
                    rc = dfol_box_positions_f32(scene->box6, 6, 6, scene->O, static_cast<float*>(at(workspace, a[1])), a[2], static_cast<int32_t>(a[3]), stream);
                    break;
                }
                rc = dfol_box_positions_f32(scene->features, scene->ld_features, scene->raw_cols, scene->O, static_cast<float*>(at(workspace, a[1])), a[2],
                                            static_cast<int32_t>(a[3]), stream);
                break;
            case DFOL_OP_FILL: {         // dst, count (32-bit words), bit pattern
                if (a[2] > 0) {
                    DFOL_REQUIRE(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(at(workspace, a[1])), static_cast<int>(a[3]), static_cast<size_t>(a[2]), s) == hipSuccess,
                                 "run_program[%d]: hipMemsetD32Async failed", i);
                }
                break;
            }
            case DFOL_OP_PAIR_LL: {      // uv, ld_uv, pos, ld_pos, req_col, req_tile, req_orient, K, tiles, scenes, tile dtype (DFOL_TILE_*)
                const float* uv = static_cast<const float*>(at(workspace, a[1]));
                const float* pos = static_cast<const float*>(at(workspace, a[3]));
                const int32_t* rc_ = static_cast<const int32_t*>(at(blob, a[5]));
                const int32_t* rt = static_cast<const int32_t*>(at(blob, a[6]));
                const uint8_t* ro = static_cast<const uint8_t*>(at(blob, a[7]));
                void* tiles = at(workspace, a[9]);
                const int32_t K = static_cast<int32_t>(a[8]), Qimg = static_cast<int32_t>(a[10]), tdt = static_cast<int32_t>(a[11]);
                DFOL_REQUIRE(tdt == DFOL_TILE_F32 || model->pair_kind != DFOL_PAIR_PLAIN, "run_program[%d]: bf16 tiles need a packed second layer", i);
                if (model->pair_kind == DFOL_PAIR_PLAIN) {
                    rc = dfol_pair_ll_f32(uv, a[2], model->hid1, pos, a[4], model->wg, static_cast<const float*>(model->w2), model->ld_w2, model->w2_rows, model->b2,
                                          model->hid2, model->emb_w, model->ld_e, model->emb_b, img_n_obj, obj_off, Qimg, scene->max_n, rc_, rt, ro, K, NS, -30.0f,
                                          static_cast<float*>(tiles), stream);
                    break;
                }
                if (model->pair_kind < 0 || model->pair_kind > DFOL_PAIR_F16) {
                    dfol_set_error("run_program[%d]: unknown pair kernel kind %d", i, model->pair_kind);
                    return 1;
                }
                rc = kPairImageEntry[model->pair_kind](uv, a[2], model->hid1, pos, a[4], model->wg, model->w2, model->b2, model->hid2, model->emb_w, model->ld_e,
                                                       model->emb_b, img_n_obj, obj_off, Qimg, scene->max_n, rc_, rt, ro, K, NS, -30.0f, tdt, tiles, stream);
                break;
            }
            case DFOL_OP_ATTR_LL:        // hidden, ld_hidden, pred_img, cols, P, ll
                rc = dfol_attr_ll_f32(static_cast<const float*>(at(workspace, a[1])), a[2], model->emb_in, model->emb_w, model->ld_e, model->emb_b, obj_off,
                                      static_cast<const int32_t*>(at(blob, a[3])), static_cast<const int32_t*>(at(blob, a[4])), static_cast<int32_t>(a[5]), NS, -30.0f,
                                      static_cast<float*>(at(workspace, a[6])), stream);
                break;
            case DFOL_OP_ATTR_HEAD: {    // pre1, ld_pre1, pred_img, cols, P, ll, scenes
                DFOL_REQUIRE(model->n_attribute == 2 && model->attribute[1].kind == DFOL_DENSE_HEAD_F16X2 && model->attribute[1].packed && model->attribute[1].bias,
                             "run_program[%d]: the model was not built for the fused attribute head", i);
                const DfolDenseLayer& l2 = model->attribute[1];
                rc = dfol_attr_head_h2_f32(static_cast<const float*>(at(workspace, a[1])), a[2], l2.K, l2.packed, l2.bias, l2.N, model->emb_w, model->ld_e, model->emb_b,
                                           obj_off, static_cast<int32_t>(a[7]), scene->O, static_cast<const int32_t*>(at(blob, a[3])),
                                           static_cast<const int32_t*>(at(blob, a[4])), static_cast<int32_t>(a[5]), NS, -30.0f, static_cast<float*>(at(workspace, a[6])), stream);
                break;
            }
            case DFOL_OP_OPTION_NORMALIZE:   // ll, seg_off, segments, pred_q, rank
                rc = dfol_option_normalize_f32(static_cast<float*>(at(workspace, a[1])), static_cast<const int32_t*>(at(blob, a[2])), static_cast<int32_t>(a[3]),
                                               static_cast<const int32_t*>(at(blob, a[4])), n_obj, NS, static_cast<int32_t>(a[5]), stream);
                break;
            case DFOL_OP_FILTER:         // att_in, ll, pred_q, neg, active, P, out
                rc = dfol_filter_fwd_f32(static_cast<const float*>(at(workspace, a[1])), static_cast<const float*>(at(workspace, a[2])),
                                         static_cast<const int32_t*>(at(blob, a[3])), n_obj, static_cast<const uint8_t*>(at(blob, a[4])), a[4] >= 0 ? 1 : 0,
                                         static_cast<const uint8_t*>(at(blob, a[5])), static_cast<int32_t>(a[6]), NS, static_cast<float*>(at(workspace, a[7])), stream);
                break;
            case DFOL_OP_RELATE_ONE:     // x, prev, tile, pred_q, quant_prev, neg, active, P, lone_forall_identity, out, tile dtype (DFOL_TILE_*)
                if (a[11] == DFOL_TILE_BF16) {
                    rc = dfol_relate_one_fwd_bf16(static_cast<const float*>(at(workspace, a[1])), static_cast<const float*>(at(workspace, a[2])),
                                                  static_cast<const uint16_t*>(at(workspace, a[3])), static_cast<const int32_t*>(at(blob, a[4])), n_obj,
                                                  static_cast<const float*>(at(blob, a[5])), static_cast<const uint8_t*>(at(blob, a[6])), a[6] >= 0 ? 1 : 0,
                                                  static_cast<const uint8_t*>(at(blob, a[7])), static_cast<int32_t>(a[8]), NS, static_cast<int32_t>(a[9]),
                                                  static_cast<float*>(at(workspace, a[10])), stream);
                    break;
                }
                rc = dfol_relate_one_fwd_f32(static_cast<const float*>(at(workspace, a[1])), static_cast<const float*>(at(workspace, a[2])),
                                             static_cast<const float*>(at(workspace, a[3])), static_cast<const int32_t*>(at(blob, a[4])), n_obj,
                                             static_cast<const float*>(at(blob, a[5])), static_cast<const uint8_t*>(at(blob, a[6])), a[6] >= 0 ? 1 : 0,
                                             static_cast<const uint8_t*>(at(blob, a[7])), static_cast<int32_t>(a[8]), NS, static_cast<int32_t>(a[9]),
                                             static_cast<float*>(at(workspace, a[10])), stream);
                break;
            case DFOL_OP_RELATE:         // prior_s, prior_o, tile, pred_q, quant_s, quant_o, neg, active, want, P, orientation, flags, post_s, post_o
                rc = dfol_relate_fwd_f32(static_cast<const float*>(at(workspace, a[1])), static_cast<const float*>(at(workspace, a[2])),
                                         static_cast<const float*>(at(workspace, a[3])), static_cast<const int32_t*>(at(blob, a[4])), n_obj,
                                         static_cast<const float*>(at(blob, a[5])), static_cast<const float*>(at(blob, a[6])), static_cast<const uint8_t*>(at(blob, a[7])),
                                         a[7] >= 0 ? 1 : 0, static_cast<const uint8_t*>(at(blob, a[8])), static_cast<const uint8_t*>(at(blob, a[9])), static_cast<int32_t>(a[10]), NS,
                                         static_cast<int32_t>(a[11]), static_cast<int32_t>(a[12]), static_cast<float*>(at(workspace, a[13])), static_cast<float*>(at(workspace, a[14])),
                                         stream);
                break;
            case DFOL_OP_FILTER_GATE:    // DFOL_OP_FILTER's operands, gate slot
                DFOL_GATE_SLOT(a[8], 1);
                rc = dfol_filter_gate_fwd_f32(static_cast<const float*>(at(workspace, a[1])), static_cast<const float*>(at(workspace, a[2])),
                                              static_cast<const int32_t*>(at(blob, a[3])), n_obj, static_cast<const uint8_t*>(at(blob, a[4])), a[4] >= 0 ? 1 : 0,
                                              static_cast<const uint8_t*>(at(blob, a[5])), static_cast<int32_t>(a[6]), NS, gate_row(a[8], 0),
                                              static_cast<float*>(at(workspace, a[7])), stream);
                break;
            case DFOL_OP_RELATE_ONE_GATE: // DFOL_OP_RELATE_ONE's operands, x_is_subject, the cell's first gate slot
                DFOL_GATE_SLOT(a[13], 2);
                DFOL_REQUIRE(a[11] == DFOL_TILE_F32 || a[11] == DFOL_TILE_BF16, "run_program[%d]: the gated relate reads fp32 or bf16 tiles", i);
                if (a[11] == DFOL_TILE_BF16) {
                    DFOL_REQUIRE(model->pair_kind != DFOL_PAIR_PLAIN, "run_program[%d]: bf16 tiles need a packed second layer", i);
                    DFOL_REQUIRE(NS % 8 == 0, "run_program[%d]: the gated relate on bf16 tiles needs NS %% 8 == 0 (NS=%d)", i, NS);
                    rc = dfol_relate_one_gate_fwd_bf16(static_cast<const float*>(at(workspace, a[1])), static_cast<const float*>(at(workspace, a[2])),
                                                       static_cast<const uint16_t*>(at(workspace, a[3])), static_cast<const int32_t*>(at(blob, a[4])), n_obj,
                                                       static_cast<const float*>(at(blob, a[5])), static_cast<const uint8_t*>(at(blob, a[12])),
                                                       static_cast<const uint8_t*>(at(blob, a[6])), a[6] >= 0 ? 1 : 0, static_cast<const uint8_t*>(at(blob, a[7])),
                                                       static_cast<int32_t>(a[8]), NS, static_cast<int32_t>(a[9]), gate_row(a[13], 0), gate_row(a[13], 1),
                                                       static_cast<float*>(at(workspace, a[10])), stream);
                    break;
                }
                rc = dfol_relate_one_gate_fwd_f32(static_cast<const float*>(at(workspace, a[1])), static_cast<const float*>(at(workspace, a[2])),
                                                  static_cast<const float*>(at(workspace, a[3])), static_cast<const int32_t*>(at(blob, a[4])), n_obj,
                                                  static_cast<const float*>(at(blob, a[5])), static_cast<const uint8_t*>(at(blob, a[12])),
                                                  static_cast<const uint8_t*>(at(blob, a[6])), a[6] >= 0 ? 1 : 0, static_cast<const uint8_t*>(at(blob, a[7])),
                                                  static_cast<int32_t>(a[8]), NS, static_cast<int32_t>(a[9]), gate_row(a[13], 0), gate_row(a[13], 1),
                                                  static_cast<float*>(at(workspace, a[10])), stream);
                break;
            case DFOL_OP_RELATE_GATE:    // DFOL_OP_RELATE's operands, the cell's first gate slot
                DFOL_GATE_SLOT(a[15], 2);
                rc = dfol_relate_gate_fwd_f32(static_cast<const float*>(at(workspace, a[1])), static_cast<const float*>(at(workspace, a[2])),
                                              static_cast<const float*>(at(workspace, a[3])), static_cast<const int32_t*>(at(blob, a[4])), n_obj,
                                              static_cast<const float*>(at(blob, a[5])), static_cast<const float*>(at(blob, a[6])),
                                              static_cast<const uint8_t*>(at(blob, a[7])), a[7] >= 0 ? 1 : 0, static_cast<const uint8_t*>(at(blob, a[8])),
                                              static_cast<const uint8_t*>(at(blob, a[9])), static_cast<int32_t>(a[10]), NS, static_cast<int32_t>(a[11]),
                                              static_cast<int32_t>(a[12]), gate_row(a[15], 0), gate_row(a[15], 1), static_cast<float*>(at(workspace, a[13])),
                                              static_cast<float*>(at(workspace, a[14])), stream);
                break;
            case DFOL_OP_QUANTIFY:       // att, quant, pred_q, P, lp
                rc = dfol_quantify_fwd_f32(static_cast<const float*>(at(workspace, a[1])), static_cast<const float*>(at(blob, a[2])),
                                           static_cast<const int32_t*>(at(blob, a[3])), n_obj, static_cast<int32_t>(a[4]), NS, static_cast<float*>(at(workspace, a[5])), stream);
                break;
            case DFOL_OP_GATE:           // x, y, x_quant, y_quant, g, P, out, out_quant
                rc = dfol_gate_f32(static_cast<const float*>(at(workspace, a[1])), static_cast<const float*>(at(workspace, a[2])), static_cast<const float*>(at(blob, a[3])),
                                   static_cast<const float*>(at(blob, a[4])), static_cast<const float*>(at(blob, a[5])), static_cast<int32_t>(a[6]), NS,
                                   static_cast<float*>(at(workspace, a[7])), static_cast<float*>(at(workspace, a[8])), stream);
                break;
            case DFOL_OP_LOGIC:          // op, a, b, n, out
                rc = dfol_logic_f32(static_cast<int32_t>(a[1]), static_cast<const float*>(at(workspace, a[2])), static_cast<const float*>(at(workspace, a[3])), a[4],
                                    static_cast<float*>(at(workspace, a[5])), stream);
                break;
            case DFOL_OP_SEGMENT_SUM_ROWS:   // src, seg_off, Q, width, out
                rc = dfol_segment_sum_rows_f32(static_cast<const float*>(at(workspace, a[1])), static_cast<const int32_t*>(at(blob, a[2])), static_cast<int32_t>(a[3]),
                                               static_cast<int32_t>(a[4]), static_cast<float*>(at(workspace, a[5])), stream);
                break;
            case DFOL_OP_SEGMENT_OR:     // lp, seg_off, Q, out, as the reference writes it (1) or in the complement form (0)
                rc = (a[5] ? dfol_segment_or_ref_f32 : dfol_segment_or_f32)(static_cast<const float*>(at(workspace, a[1])), static_cast<const int32_t*>(at(blob, a[2])),
                                                                            static_cast<int32_t>(a[3]), static_cast<float*>(at(workspace, a[4])), stream);
                break;
            case DFOL_OP_IMPLICATION:    // prior, x, pred_q, P, out
                rc = dfol_implication_f32(static_cast<const float*>(at(workspace, a[1])), static_cast<const float*>(at(workspace, a[2])),
                                          static_cast<const int32_t*>(at(blob, a[3])), n_obj, static_cast<int32_t>(a[4]), NS, static_cast<float*>(at(workspace, a[5])), stream);
                break;
            case DFOL_OP_COMPARE:        // lp1, lp2, is_less, Q, out
                rc = dfol_compare_f32(static_cast<const float*>(at(workspace, a[1])), static_cast<const float*>(at(workspace, a[2])), static_cast<const float*>(at(blob, a[3])),
                                      static_cast<int32_t>(a[4]), static_cast<float*>(at(workspace, a[5])), stream);
                break;
            case DFOL_OP_FIND_MAX_IND: { // lp, seg_off, Q, threshold (float bits), flags
                float thr;
                const int32_t bits = static_cast<int32_t>(a[4]);
                memcpy(&thr, &bits, 4);
                rc = dfol_find_max_ind_f32(static_cast<const float*>(at(workspace, a[1])), static_cast<const int32_t*>(at(blob, a[2])), static_cast<int32_t>(a[3]), thr,
                                           static_cast<uint8_t*>(at(workspace, a[5])), stream);
                break;
            }
            case DFOL_OP_GATHER_TILES:   // src rows, index, count, dst rows, width in 32-bit words (0: NS * NS): dst[p] = src[index[p]] - shared scenes (one tile per distinct
                                         // (scene, concept, orientation); bf16 tiles are NS * NS / 2 words), compacted option lists, LSTM states by question
                rc = dfol_gather_rows_f32(static_cast<const float*>(at(workspace, a[1])), static_cast<const int32_t*>(at(blob, a[2])), static_cast<int32_t>(a[3]),
                                          a[5] > 0 ? static_cast<int32_t>(a[5]) : NS * NS, static_cast<float*>(at(workspace, a[4])), stream);
                break;
            case DFOL_OP_CALIB_FEATURES: // head, n_head, table, E, idx, P, out
                rc = dfol_calib_features_f32(static_cast<const float*>(at(blob, a[1])), static_cast<int32_t>(a[2]), static_cast<const float*>(at(blob, a[3])),
                                             static_cast<int32_t>(a[4]), static_cast<const int32_t*>(at(blob, a[5])), static_cast<int32_t>(a[6]),
                                             static_cast<float*>(at(workspace, a[7])), stream);
                break;
            case DFOL_OP_LSTM_CELL: {    // which, x (-1: built from tokens), h, c, rows, h_out, c_out; then head, n_head, table, E, idx
                const int w = a[1] ? 1 : 0;
                DFOL_REQUIRE(model->lstm_wih_t[w] && model->lstm_whh_t[w] && model->lstm_h > 0 && model->lstm_kx > 0, "run_program[%d]: the model has no calibration LSTM", i);
                if (a[2] < 0) {
                    DFOL_REQUIRE(a[9] + a[11] == model->lstm_kx, "run_program[%d]: token rows of %lld floats for an LSTM of input width %d", i,
                                 (long long)(a[9] + a[11]), model->lstm_kx);
                    rc = dfol_lstm_cell_tokens_f32(static_cast<const float*>(at(blob, a[8])), static_cast<int32_t>(a[9]), static_cast<const float*>(at(blob, a[10])),
                                                   static_cast<int32_t>(a[11]), static_cast<const int32_t*>(at(blob, a[12])),
                                                   static_cast<const float*>(at(workspace, a[3])), model->lstm_h, static_cast<const float*>(at(workspace, a[4])),
                                                   model->lstm_wih_t[w], model->lstm_ld_wih[w], model->lstm_whh_t[w], model->lstm_ld_whh[w], model->lstm_bih[w],
                                                   model->lstm_bhh[w], static_cast<int32_t>(a[5]), model->lstm_h, static_cast<float*>(at(workspace, a[6])),
                                                   static_cast<float*>(at(workspace, a[7])), stream);
                    break;
                }
                rc = dfol_lstm_cell_f32(static_cast<const float*>(at(workspace, a[2])), model->lstm_kx, model->lstm_kx, static_cast<const float*>(at(workspace, a[3])),
                                        model->lstm_h, static_cast<const float*>(at(workspace, a[4])), model->lstm_wih_t[w], model->lstm_ld_wih[w], model->lstm_whh_t[w],
                                        model->lstm_ld_whh[w], model->lstm_bih[w], model->lstm_bhh[w], static_cast<int32_t>(a[5]), model->lstm_h,
                                        static_cast<float*>(at(workspace, a[6])), static_cast<float*>(at(workspace, a[7])), stream);
                break;
            }
            case DFOL_OP_SELECT_ROWS:    // x, y, flags, P, width, out
                rc = dfol_select_rows_f32(static_cast<const float*>(at(workspace, a[1])), static_cast<const float*>(at(workspace, a[2])),
                                          static_cast<const uint8_t*>(at(blob, a[3])), static_cast<int32_t>(a[4]), static_cast<int32_t>(a[5]),
                                          static_cast<float*>(at(workspace, a[6])), stream);
                break;
            case DFOL_OP_ATT_MODULATIONS: // fs, bs, P, out
                DFOL_REQUIRE(model->att_out_w && model->att_out_n > 0, "run_program[%d]: the model has no attention-output network", i);
                rc = dfol_attention_modulations_f32(static_cast<const float*>(at(workspace, a[1])), static_cast<const float*>(at(workspace, a[2])), model->att_out_w,
                                                    model->ld_att_out, model->att_out_b, static_cast<int32_t>(a[3]), model->lstm_h, model->att_out_n,
                                                    static_cast<float*>(at(workspace, a[4])), stream);
                break;
            case DFOL_OP_CALIB_WALK:     // table of DFOL_WALK_* steps (blob), steps, rows
                rc = run_calib_walk(model, static_cast<const int64_t*>(at(blob, a[1])), static_cast<int32_t>(a[2]), static_cast<int32_t>(a[3]), workspace, blob, stream);
                break;
            case DFOL_OP_MODULATE:       // att, mods, pred_q, P, out
                DFOL_REQUIRE(model->att_out_n == 4, "run_program[%d]: dfol_modulate_f32 takes 4-column modulations", i);
                rc = dfol_modulate_f32(static_cast<const float*>(at(workspace, a[1])), static_cast<const float*>(at(workspace, a[2])),
                                       static_cast<const int32_t*>(at(blob, a[3])), n_obj, static_cast<int32_t>(a[4]), NS, static_cast<float*>(at(workspace, a[5])), stream);
                break;
            default:
                dfol_set_error("run_program[%d]: unknown opcode %lld", i, (long long)a[0]);
                return 1;
        }
        if (rc != 0) {
            char msg[480];
            snprintf(msg, sizeof(msg), "%s", dfol_last_error());
            dfol_set_error("run_program: instruction %d (opcode %lld): %s", i, (long long)a[0], msg);
            return rc;
        }
    }
#undef DFOL_GATE_SLOT
    return 0;
}
