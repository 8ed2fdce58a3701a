// sequence_engine.h -- lock-step batch of alignments for an odometry sequence (BASELINE.json configs[3]; the per-GPU engine behind
// rgbd360_align360_batch[_dev] and the multi-GPU entry).  Included by rgbd360_api.hip.
//
// A 4-level alignment is ~35 dependent launches, most of them over 32 K - 500 K pixels: pure launch latency on a 256-CU part.
// The engine keeps P pairs ("slots") in flight on ONE stream and gives every launch a slot dimension: one k_eval_b /
// k_solve_b per {level, iteration} serves all P pairs (each slot gated by its own device-resident GNState, exactly like the
// one-pair kernels), and the frame set-up kernels convert / reduce / differentiate the P new frames of a round together.  The
// cost of a round of P alignments is then the launch count of ONE alignment plus P times the bandwidth-bound work.
//
// Slot s owns the contiguous pairs [a_s, b_s) of the sequence (frame reuse inside the span: the source of pair j is the target
// of pair j+1, its planes change role and only its gradient records are built); round r aligns pair a_s + r in every slot that
// still has one (live mask).  Work split, partial rows and summation order per slot are those of the one-pair path
// (RPI.h:4519-4784 semantics unchanged): poses are bit-identical to rgbd360_align360 pair by pair.
#pragma once

namespace {

struct SeqLevel : LevelGeom {      // geometry, tables and work split as a one-pair context has them (level_geom.h)
    DevBuf<float> gray, depth;                    // [P][n] planes of levels >= 1 (level 0 is never stored)
    DevBuf<float4> srcRec;                        // [P][n]
    DevBuf<F3> trgP[2], trgD[2];                  // [P][n] x 2: the records of a frame are built when it arrives as a source, one round
                                                  // before it is the target
    DevBuf<float> sinT, cosT, sinP, cosP;
    DevBuf<float2> tabT, tabP;                    // interleaved {sin, cos} (recompute form of the pass)
    bool compact = false;                         // source records of this level are {depth, Isrc} (8 B) and k_eval_b re-forms the point
};

// Frame-store mode of an engine (frame_store.h): the records of a level are not the engine's [P][n] slot buffers but the store's
// [capacity][n] entry arrays, and slot s of a round aligns entry pt.trg[s] (target) with entry pt.src[s] (source) from its own guess.
struct StoreLevelView {                   // non-owning: the arrays belong to the store (rgbd360_store::entries)
    float4* src = nullptr;                // [capacity][n] source records (16 B, or 8 B on a compact level)
    F3 *trgP = nullptr, *trgD = nullptr;  // [capacity][n]
};
struct StoreView {
    std::vector<StoreLevelView> levels;
    PairTable pt;                         // the pairs of the round in flight (parked slots: entry 0)
    DevBuf<Pose16> d_guess;               // [P] start poses of the round, filled by one async copy in front of it ...
    PinnedBuf<Pose16> h_guess;            // ... from this pinned array (default flags)
};

struct SeqEngine {
    rgbd360_params p;
    int P = 0, rows = 0, cols = 0;
    hipStream_t stream = nullptr;
    UploadRing ring;                  // host-frame sequences: [P] packed frames per slot, frame s at s * frame_bytes(bytes per pixel)
    std::vector<SeqLevel> levels;
    DevBuf<GNState> d_states;
    PinnedBuf<GNState> h_states{hostwait::kPublishedFlags};
    DevBuf<double> d_partials;
    int partials_stride = 0;          // doubles per slot
    size_t frame_bytes(size_t px_bytes) const { return (size_t)rows * cols * px_bytes; }
    int tb = 0;                       // which target-record buffer holds the TARGETS of the round
    int max_eval_blocks = 256;
    int libm = 0;                 // the warp in the reference's libm arithmetic (the owning context's rgbd360_set_index_arithmetic)
    int chunk_top = 8, chunk_mid = 4, chunk_l0 = 4;      // {pass, solve} pairs enqueued ahead per level and visit
    StoreView* sv = nullptr;          // frame-store mode (owned by the store, not by the engine)
    std::string err;
};

#define SEQC(E, expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess) {                                                         \
            (E)->err = std::string(#expr) + ": " + hipGetErrorString(e_);               \
            return -(int)e_ - 1000;                                                     \
        }                                                                               \
    } while (0)

void seq_free(SeqEngine* E) {
    if (!E) return;
    hipSetDevice(E->p.device);
    if (E->stream) hipStreamSynchronize(E->stream);
    upload_ring_destroy(E->ring);
    if (E->stream) hipStreamDestroy(E->stream);
    delete E;      // every buffer of the engine and of its levels
}

// alloc: kSeqPlanes = the [P][n] float planes of levels >= 1, kSeqRecords = the [P][n] record buffers.  A frame store's engines
// leave out what the store holds per entry (frame_store.h).
enum { kSeqPlanes = 1, kSeqRecords = 2 };
int seq_create(const rgbd360_params& p, int P, int rows, int cols, int max_eval_blocks, SeqEngine** out, std::string* err,
               int alloc = kSeqPlanes | kSeqRecords) {
    *out = nullptr;
    if (P < 1 || P > kMaxSlots) { *err = "slots per engine must be in 1..32"; return -1; }
    if (const char* why = check_image_size(p, rows, cols)) { *err = why; return -1; }
    if (hipSetDevice(p.device) != hipSuccess) { *err = "hipSetDevice failed"; return -102; }
    SeqEngine* E = new SeqEngine();
    E->p = p; E->P = P; E->rows = rows; E->cols = cols; E->max_eval_blocks = max_eval_blocks;
    if (const char* e = knobs::debug("RGBD360_SEQ_CHUNKS")) {        // "top,mid,l0" tuning knob
        int a = 0, b = 0, c = 0;
        if (sscanf(e, "%d,%d,%d", &a, &b, &c) == 3 && a >= 1 && a <= 16 && b >= 1 && b <= 16 && c >= 1 && c <= 16) {
            E->chunk_top = a; E->chunk_mid = b; E->chunk_l0 = c;
        }
    }
    auto bad = [&](const char* what) {
        *err = what;
        seq_free(E);
        return -103;
    };
    if (hipStreamCreateWithFlags(&E->stream, hipStreamNonBlocking) != hipSuccess) return bad("cannot create the engine's stream");
    E->levels.resize(p.n_pyr);
    int r = rows, c = cols, max_blocks = 0;
    for (int l = 0; l < p.n_pyr; ++l) {
        SeqLevel& L = E->levels[l];
        static_cast<LevelGeom&>(L) = level_geom(r, c, max_eval_blocks);
        const size_t np = (size_t)P * L.n;
        bool ok = true;
        auto need = [&ok](auto& buf, size_t count) { ok = ok && buf.ensure(count) == hipSuccess; };
        if (l > 0 && (alloc & kSeqPlanes)) { need(L.gray, np); need(L.depth, np); }
        if (alloc & kSeqRecords) {
            need(L.srcRec, np);
            for (int k = 0; k < 2; ++k) { need(L.trgP[k], np); need(L.trgD[k], np); }
        }
        need(L.sinT, c); need(L.cosT, c); need(L.sinP, r); need(L.cosP, r);
        if (!ok) return bad("out of device memory for the sequence engine");
        if (L.tabT.ensure(c) != hipSuccess || L.tabP.ensure(r) != hipSuccess ||
            upload_angle_tables(angle_tables(L), L.sinT, L.cosT, L.sinP, L.cosP, L.tabT, L.tabP) != hipSuccess)
            return bad("table upload failed");
        // The engine's launches serve P pairs at once, so its large levels are fed from HBM whatever the image size: they carry the
        // 8-byte {depth, Isrc} source record and k_eval_b re-forms the point (SrcForm<2>: 32 instead of 40 B/px per pass, 32 instead of
        // 40 B/px written by the set-up).  The latency-bound small levels keep the 16-byte record.  RGBD360_SEQ_RECOMPUTE_MIN_PX moves
        // the bound (0: every level; a huge value: none).  The rig's pinhole records never take this form (rig_dense.h builds its own).
        static const int seq_min_px = [] { const char* e = knobs::product("RGBD360_SEQ_RECOMPUTE_MIN_PX"); return e ? atoi(e) : 256 * 1024; }();
        L.compact = L.n >= seq_min_px;
        max_blocks = std::max(max_blocks, L.nblocks);
        r /= 2; c /= 2;
    }
    E->partials_stride = max_blocks * kNumPartials;
    if (E->d_partials.ensure((size_t)P * E->partials_stride) != hipSuccess || E->d_states.ensure(P) != hipSuccess ||
        hipMemset(E->d_states, 0, (size_t)P * sizeof(GNState)) != hipSuccess || E->h_states.ensure(P) != hipSuccess)
        return bad("out of memory for the engine state");
    *out = E;
    return 0;
}

LevelDev seq_level_dev(const SeqLevel& L, int tb) {
    LevelDev d;
    fill_level_dev(d, L);
    d.src = L.srcRec; d.trgP = L.trgP[tb]; d.trgD = L.trgD[tb];
    d.src2 = reinterpret_cast<const float2*>(L.srcRec.get()); d.tabT = L.tabT; d.tabP = L.tabP;
    return d;
}

void seq_launch_eval(SeqEngine* E, int level, int method) {
    const SeqLevel& L = E->levels[level];
    LevelDev lv = seq_level_dev(L, E->tb);
    lv.min_depth = E->p.min_depth; lv.max_depth = E->p.max_depth;
    lv.libm = E->libm;
    const EvalConsts ec = eval_consts(E->p);
    const dim3 g(L.nblocks, E->P), b(kEvalThreadsBatch);
    if (E->sv) {
        const StoreLevelView& V = E->sv->levels[level];
        lv.src = V.src; lv.src2 = reinterpret_cast<const float2*>(V.src); lv.trgP = V.trgP; lv.trgD = V.trgD;
    }
    with_choice<0, 2>(L.compact, [&](auto S) {
        with_method(method, [&](auto M) {
            if (E->sv)
                hipLaunchKernelGGL((k_eval_p<M, true, S>), g, b, 0, E->stream, E->d_states.get(), lv.src, lv.n, L.chunk, level, L.nblocks, E->d_partials.get(),
                                   E->partials_stride, lv, ec, E->sv->pt);
            else
                hipLaunchKernelGGL((k_eval_b<M, true, S>), g, b, 0, E->stream, E->d_states.get(), lv.src, lv.n, L.chunk, level, L.nblocks, E->d_partials.get(),
                                   E->partials_stride, lv, ec);
        });
    });
}

void seq_launch_solve(SeqEngine* E, int level, int forced = 0) {
    const SeqLevel& L = E->levels[level];
    SolveCfg cfg;
    cfg.level = level; cfg.mode = 0; cfg.forced = forced; cfg.max_iters = E->p.max_iters; cfg.n_pixels = L.n;
    cfg.occ = 0;
    cfg.tol_residual = E->p.tol_residual; cfg.tol_update = E->p.tol_update;
    hipLaunchKernelGGL(k_solve_b, dim3(E->P), dim3(kSolveThreads), 0, E->stream, E->d_states.get(), E->d_partials.get(), E->partials_stride, L.nblocks, cfg);
}

// guess: the start pose of every slot; a frame-store engine takes one pose per slot from sv->d_guess instead.
void seq_enqueue_schedule(SeqEngine* E, int pending, bool pending_started, const float* guess, int method, unsigned long long live) {
    const int top = E->p.n_pyr - 1;
    for (int level = pending; level >= 0; --level) {
        if (level == top && !pending_started) {
            if (E->sv) {
                hipLaunchKernelGGL(k_level_init_p, dim3(E->P), dim3(64), 0, E->stream, E->d_states.get(), E->sv->d_guess.get(), 1, 1, level, live);
            } else {
                Pose16 Pz;
                memcpy(Pz.v, guess, sizeof(Pz.v));
                hipLaunchKernelGGL(k_level_init_b, dim3(E->P), dim3(64), 0, E->stream, E->d_states.get(), Pz, 1, 1, level, live);
            }
        }
        const int n_pairs = (level == top && !pending_started) ? E->chunk_top : (level == 0 ? E->chunk_l0 : E->chunk_mid);
        for (int k = 0; k < n_pairs; ++k) {
            seq_launch_eval(E, level, method);
            seq_launch_solve(E, level);
        }
    }
}

// One frame per live slot through the fused set-up (k_frame_level_b, one launch per pyramid level): source records for the slots
// of src_mask, target records (into buffer trg_buf) for those of trg_mask, next-level planes for all.
// store / et (frame store): the records of slot s go to entry et->e[s] of the store's arrays instead (k_frame_level_e).
void seq_frame_setup(SeqEngine* E, const FramePtrs& fp, size_t rgb_step, size_t depth_step, int depth_type, unsigned long long live,
                     unsigned long long src_mask, unsigned long long trg_mask, int trg_buf, const StoreView* store = nullptr,
                     const EntryTable* et = nullptr) {
    for (int l = 0; l < E->p.n_pyr; ++l) {
        const SeqLevel& L = E->levels[l];
        FrameLevelArgs A;
        memset(&A, 0, sizeof(A));
        A.rows = L.rows; A.cols = L.cols;
        if (l + 1 < E->p.n_pyr) {
            const SeqLevel& N = E->levels[l + 1];
            A.drows = N.rows; A.dcols = N.cols;
            A.gray_next = N.gray; A.depth_next = N.depth;
        }
        A.seam = E->p.mask_seams ? L.cols / 8 : 0;
        A.depth_type = depth_type;
        A.rgb_step = rgb_step; A.depth_step = depth_step;
        A.gray_in = L.gray; A.depth_in = L.depth;
        A.src_rec = L.srcRec; A.trg_p = L.trgP[trg_buf]; A.trg_d = L.trgD[trg_buf];
        if (store) { A.src_rec = store->levels[l].src; A.trg_p = store->levels[l].trgP; A.trg_d = store->levels[l].trgD; }
        A.sin_theta = L.sinT; A.cos_theta = L.cosT; A.sin_phi = L.sinP; A.cos_phi = L.cosP;
        A.min_depth = E->p.min_depth; A.max_depth = E->p.max_depth;
        A.compact_src = L.compact ? 1 : 0;
        A.live_mask = live; A.src_mask = src_mask; A.trg_mask = trg_mask;
        const dim3 g((L.cols + kFsTW - 1) / kFsTW, (L.rows + kFsTH - 1) / kFsTH, E->P);
        if (store) {
            if (l == 0) hipLaunchKernelGGL((k_frame_level_e<true>), g, dim3(256), 0, E->stream, A, fp, *et);
            else hipLaunchKernelGGL((k_frame_level_e<false>), g, dim3(256), 0, E->stream, A, fp, *et);
        } else if (l == 0) hipLaunchKernelGGL((k_frame_level_b<true>), g, dim3(256), 0, E->stream, A, fp);
        else hipLaunchKernelGGL((k_frame_level_b<false>), g, dim3(256), 0, E->stream, A, fp);
    }
}

// Both staging slots of the engine's ring for P frames of this depth type.  The image size of an engine is fixed, so only the depth
// type moves the need: the slots grow for float32 depth and stay that size for uint16 frames afterwards.
int seq_ensure_stage(SeqEngine* E, int depth_type) {
    UploadRing& U = E->ring;
    const size_t need_rgb = E->frame_bytes(3) * E->P, need_depth = E->frame_bytes(depth_type == 0 ? 2 : 4) * E->P;
    SEQC(E, U.open());
    if (U.holds(need_rgb, need_depth, 0) && U.holds(need_rgb, need_depth, 1)) return 0;
    SEQC(E, hipStreamSynchronize(E->stream));      // nothing in flight reads what is about to be freed
    SEQC(E, hipStreamSynchronize(U.stream));
    for (int k = 0; k < 2; ++k) SEQC(E, U.ensure(need_rgb, need_depth, k));
    return 0;
}

void result_from_state(const GNState& S, int n_pyr, int occ, float pose_out[16], rgbd360_result* res) {
    rgbd360_result R;
    memset(&R, 0, sizeof(R));
    for (int l = 0; l < n_pyr && l < 8; ++l) R.iters[l] = S.iters[l];
    memcpy(pose_out, S.pose, sizeof(float) * 16);
    R.status = S.status;
    memcpy(R.hessian, S.Hused, sizeof(R.hessian));
    memcpy(R.gradient, S.gused, sizeof(R.gradient));
    R.sso = S.used_npix ? (float)S.used_nvis / (float)S.used_npix : 0.f;
    const double nv = (double)(S.acc_np + S.acc_nd);
    R.err_final = nv > 0 ? sqrt((S.acc_e2p + S.acc_e2d) / nv) : 0.0;
    if (occ != 0)       // avPhotoResidual + avDepthResidual (RPI.h:3358-3366, 3848-3855)
        R.err_final = (S.acc_np > 0 ? sqrt(S.acc_e2p / (double)S.acc_np) : 0.0) + (S.acc_nd > 0 ? sqrt(S.acc_e2d / (double)S.acc_nd) : 0.0);
    R.rms_photo = S.acc_np > 0 ? sqrt(S.acc_e2p / (double)S.acc_np) : 0.0;
    R.rms_depth = S.acc_nd > 0 ? sqrt(S.acc_e2d / (double)S.acc_nd) : 0.0;
    if (res) *res = R;
}

// Waits for the round whose first schedule is enqueued: reads the slots' states back (E->h_states holds them on return) and tops the
// schedule up until every live slot has finished its finest level or carries a status.
int seq_finish_round(SeqEngine* E, int n_slots, const float* guess, int method, unsigned long long live) {
    for (int round = 0;; ++round) {
        SEQC(E, hipMemcpyAsync(E->h_states, E->d_states, (size_t)n_slots * sizeof(GNState), hipMemcpyDeviceToHost, E->stream));
        SEQC(E, hipStreamSynchronize(E->stream));
        int pending = -1;
        for (int s = 0; s < n_slots; ++s) {
            if (!((live >> s) & 1ull)) continue;
            const GNState& S = E->h_states[s];
            if (S.status != 0 || (S.level_active == 0 && S.done)) continue;
            if (S.done) { E->err = "alignment schedule stalled between levels"; return -6; }
            pending = std::max(pending, S.level_active);
        }
        if (pending < 0) return 0;
        if (round > (E->p.max_iters + 4) * E->p.n_pyr) { E->err = "alignment loop did not terminate"; return -6; }
        seq_enqueue_schedule(E, pending, true, guess, method, live);      // the stalled level gets another chunk, then the finer ones
        SEQC(E, hipGetLastError());
    }
}

// Slot s aligns the pairs [a[s], b[s]) of the sequence rgb[] / depth[] (global frame indices; pair j = frames j, j+1).
// (seq_run below wraps this body with the one exit that matters: whatever the outcome, no copy from the caller's images and no
// launch of this call is still in flight when the C call returns.)
int seq_run_body(SeqEngine* E, int n_slots, const int* a, const int* b, const uint8_t* const* rgb, size_t rgb_step, const void* const* depth,
            size_t depth_step, int depth_type, const float* guess, int method, bool on_device, float* poses_out, rgbd360_result* results_out) {
    hipSetDevice(E->p.device);
    const int P = E->P;
    if (n_slots < 1 || n_slots > P) { E->err = "bad slot count"; return -1; }
    int rounds = 0;
    for (int s = 0; s < n_slots; ++s) rounds = std::max(rounds, b[s] - a[s]);
    if (rounds == 0) return 0;
    const size_t dpx = depth_type == 0 ? 2 : 4;
    const size_t fr = E->frame_bytes(3), fd = E->frame_bytes(dpx);      // a staged frame
    UploadRing& U = E->ring;
    if (!on_device) {
        const int rc = seq_ensure_stage(E, depth_type);
        if (rc) return rc;
    }
    auto live_of = [&](int r) {        // slots that still have a pair in round r
        unsigned long long m = 0;
        for (int s = 0; s < n_slots; ++s)
            if (a[s] + r < b[s]) m |= 1ull << s;
        return m;
    };
    // frames of a round: which = 0 the targets of round 0 (frame a[s]), 1 the sources of round r (frame a[s] + r + 1)
    auto frame_of = [&](int s, int r, int which) { return which == 0 ? a[s] : a[s] + r + 1; };
    // host frames travel through staging parity `par`: upload on the copy stream (after the parity's previous frames were converted)
    auto upload = [&](int r, int which, int par, unsigned long long live) -> int {
        SEQC(E, hipStreamWaitEvent(U.stream, U.conv_ev[par], 0));
        for (int s = 0; s < n_slots; ++s) {
            if (!((live >> s) & 1ull)) continue;
            const int f = frame_of(s, r, which);
            SEQC(E, copy_frame_h2d(U.rgb[par] + s * fr, U.depth[par] + s * fd, rgb[f], rgb_step, depth[f], depth_step, depth_type, E->rows, E->cols,
                                   U.stream));
        }
        SEQC(E, hipEventRecord(U.up_ev[par], U.stream));
        return 0;
    };
    auto frame_ptrs = [&](int r, int which, int par, unsigned long long live, FramePtrs* fp, size_t* rs, size_t* ds) {
        memset(fp, 0, sizeof(*fp));
        for (int s = 0; s < n_slots; ++s) {
            if (!((live >> s) & 1ull)) continue;
            if (on_device) {
                const int f = frame_of(s, r, which);
                fp->rgb[s] = rgb[f];
                fp->depth[s] = depth[f];
            } else {
                fp->rgb[s] = U.rgb[par] + s * fr;
                fp->depth[s] = U.depth[par] + s * fd;
            }
        }
        *rs = on_device ? rgb_step : (size_t)E->cols * 3;
        *ds = on_device ? depth_step : (size_t)E->cols * dpx;
    };
    int rc = 0;
    int par = 0;      // staging parity of the NEXT conversion
    if (!on_device) {
        if ((rc = upload(0, 0, 0, live_of(0))) != 0) return rc;      // targets of round 0 -> parity 0
        if ((rc = upload(0, 1, 1, live_of(0))) != 0) return rc;      // sources of round 0 -> parity 1
    }
    for (int r = 0; r < rounds; ++r) {
        const unsigned long long live = live_of(r);
        FramePtrs fp;
        size_t rs, ds;
        if (r == 0) {
            // first targets: frames a[s], target records only, into buffer tb
            frame_ptrs(0, 0, par, live, &fp, &rs, &ds);
            if (!on_device) SEQC(E, hipStreamWaitEvent(E->stream, U.up_ev[par], 0));
            seq_frame_setup(E, fp, rs, ds, depth_type, live, 0ull, live, E->tb);
            if (!on_device) { SEQC(E, hipEventRecord(U.conv_ev[par], E->stream)); par ^= 1; }
        }
        // sources of this round; they are the targets of the next one in every slot that has another pair: their target
        // records go into the other buffer now, while the tile is in LDS anyway
        frame_ptrs(r, 1, par, live, &fp, &rs, &ds);
        if (!on_device) SEQC(E, hipStreamWaitEvent(E->stream, U.up_ev[par], 0));
        seq_frame_setup(E, fp, rs, ds, depth_type, live, live, live & live_of(r + 1), E->tb ^ 1);
        if (!on_device) {
            SEQC(E, hipEventRecord(U.conv_ev[par], E->stream));
            par ^= 1;
        }
        seq_enqueue_schedule(E, E->p.n_pyr - 1, false, guess, method, live);
        SEQC(E, hipGetLastError());
        // next round's sources travel while this round is being aligned (a pageable-memory copy keeps the host in the call, so
        // it is issued only now that the round's launches are queued)
        if (!on_device && r + 1 < rounds && (rc = upload(r + 1, 1, par, live_of(r + 1))) != 0) return rc;
        if ((rc = seq_finish_round(E, n_slots, guess, method, live)) != 0) return rc;
        for (int s = 0; s < n_slots; ++s) {
            if (!((live >> s) & 1ull)) continue;
            const int j = a[s] + r;
            result_from_state(E->h_states[s], E->p.n_pyr, 0, poses_out + (size_t)16 * j, results_out ? &results_out[j] : nullptr);
        }
        E->tb ^= 1;      // this round's sources are the next round's targets
    }
    if (U.stream) SEQC(E, hipStreamSynchronize(U.stream));      // no upload may outlive the caller's buffers
    return 0;
}

int seq_run(SeqEngine* E, int n_slots, const int* a, const int* b, const uint8_t* const* rgb, size_t rgb_step, const void* const* depth,
            size_t depth_step, int depth_type, const float* guess, int method, bool on_device, float* poses_out, rgbd360_result* results_out) {
    const int rc = seq_run_body(E, n_slots, a, b, rgb, rgb_step, depth, depth_step, depth_type, guess, method, on_device, poses_out, results_out);
    if (rc != 0) {
        // an error return left the body early: hipMemcpy2DAsync copies from the caller's host images may still be queued on the copy
        // stream, staged frames unconverted and event waits pending on the engine's stream.  Drain both (errors here change nothing:
        // the call already failed) so that the caller may free its buffers and the kept engine starts its next call clean.
        if (E->ring.stream) (void)hipStreamSynchronize(E->ring.stream);
        if (E->stream) (void)hipStreamSynchronize(E->stream);
    }
    return rc;
}

}  // namespace
