// frame_store.h -- a resident store of PREPARED frames and the lock-step alignment of arbitrary pairs of them (rgbd360_store_*,
// include/rgbd360_hip.h).  Included by rgbd360_api.hip behind sequence_engine.h.
//
// The sequence engine aligns the consecutive pairs of a sequence from one guess: slot s reads the records slot s itself built one
// round earlier.  Every other caller of alignFrames360 in the reference aligns pairs that are not consecutive, each from its own
// guess: a keyframe against every following frame (OdometryKeyFrame360.cpp:244-253), the nearest keyframe against the current frame
// (KFsphere_SLAM.cpp:146-150, 370-375), a new keyframe against several old ones in both roles (LoopClosure360.h:309-312, 348-351).
// Here a frame is prepared ONCE, when it is put into the store -- for every pyramid level its source records and both target record
// streams, the three streams the per-pixel pass reads -- and an align call runs a list of (target entry, source entry,
// guess) triples through the engine's lock-step schedule, P pairs per round, each launch serving all P pairs.
//
// Layout: per level three arrays over all entries, srcRec[capacity][n] (16 B per pixel, 8 B on the levels the engine keeps compact),
// trgP[capacity][n] and trgD[capacity][n] (12 B each).  The pass finds its two entries through a table in the kernel arguments
// (k_eval_p), the set-up writes through one (k_frame_level_e); the bodies are the engine's, so every pair's result carries the bits
// rgbd360_align360 gives for the same two frames and guess.
//
// Shared with the sequence engine (sequence_engine.h, nothing forked): geometry / tables / work split (seq_create, without the
// buffers the store holds per entry), the fused set-up's launch code (seq_frame_setup), the chunked speculative schedule
// (seq_enqueue_schedule), the read-back and top-up loop (seq_finish_round), k_solve_b and result_from_state.
//
// Out of scope: occlusion modes 1 / 2 (the z-buffer passes have no slot dimension), the pinhole and rig paths, several GPUs
// (rgbd360_multi_*), an eviction policy (the caller chooses which entry to overwrite), PbMap (the guess is an input).
#pragma once

struct rgbd360_store {
    rgbd360_ctx* ctx = nullptr;
    rgbd360_params p;
    int capacity = 0, rows = 0, cols = 0, max_eval_blocks = 256;
    struct Entries {                      // one level's [capacity][n] arrays
        DevBuf<float2> src;               // source records: one float2 per pixel on a compact level, two (a float4) otherwise
        DevBuf<F3> trgP, trgD;
    };
    std::vector<Entries> entries;         // owned here; `view` and the engines' views point into them
    StoreView view;                       // the entry arrays (view.levels); pt / guesses unused here
    std::vector<char> occupied;
    size_t entry_bytes = 0;
    SeqEngine* put_eng = nullptr;         // set-up: up to 32 frames per launch; owns the [P][n] plane scratch of levels >= 1 and the staging
    SeqEngine* eng[2] = {nullptr, nullptr};      // alignment: states, partial rows and stream of up to 2 x 32 slots, no frame buffers
    StoreView eng_view[2];
    int n_eng = 0;
    DevBuf<unsigned char> ov_table, ov_segs;      // store_overlap.h: the pair table (and its per-source segments) of a call and ...
    DevBuf<int32_t> ov_counts;            // ... its [records][8] counters, both on put_eng's stream
    std::string err;
};

namespace {

int store_fail(rgbd360_store* st, int code, const std::string& msg) {
    st->err = msg;
    return code;
}

void store_free_engines(rgbd360_store* st) {
    for (int e = 0; e < 2; ++e) {
        if (st->eng[e]) seq_free(st->eng[e]);      // drains the engine's stream first
        st->eng[e] = nullptr;
        st->eng_view[e].d_guess.release();
        st->eng_view[e].h_guess.release();
    }
    st->n_eng = 0;
}

void store_free(rgbd360_store* st) {
    if (!st) return;
    hipSetDevice(st->p.device);
    store_free_engines(st);
    if (st->put_eng) seq_free(st->put_eng);
    delete st;      // the entry arrays: nothing of an engine is left to read them
}

// n_eng engines of P slots each, kept between calls
int store_ensure_engines(rgbd360_store* st, int n_eng, int P) {
    if (st->n_eng == n_eng && st->eng[0] && st->eng[0]->P == P) return 0;
    store_free_engines(st);
    for (int e = 0; e < n_eng; ++e) {
        std::string err;
        const int rc = seq_create(st->p, P, st->rows, st->cols, st->max_eval_blocks, &st->eng[e], &err, 0);
        if (rc) { store_free_engines(st); return store_fail(st, rc, err); }
        StoreView& V = st->eng_view[e];
        V.levels = st->view.levels;
        memset(&V.pt, 0, sizeof(V.pt));
        if (V.d_guess.ensure(P) != hipSuccess || V.h_guess.ensure(P) != hipSuccess) {
            store_free_engines(st);
            return store_fail(st, -103, "out of memory for the store's alignment engines");
        }
        st->eng[e]->sv = &V;
        st->n_eng = e + 1;
    }
    return 0;
}

// The pairs [lo, hi) of the list on one engine, n_slots per round in list order; the last round is partial under the live mask.
int store_run_engine(SeqEngine* E, int n_slots, int lo, int hi, const int* trg, const int* src, const float* guesses, int method,
                     float* poses_out, rgbd360_result* results_out) {
    hipSetDevice(E->p.device);
    StoreView& V = *E->sv;
    for (int k = lo; k < hi; k += n_slots) {
        const int m = std::min(n_slots, hi - k);
        const unsigned long long live = m >= 64 ? ~0ull : (1ull << m) - 1;
        for (int s = 0; s < kMaxSlots; ++s) {      // a parked slot still issues its first record loads: entry 0 is memory of the store
            V.pt.trg[s] = s < m ? trg[k + s] : 0;
            V.pt.src[s] = s < m ? src[k + s] : 0;
        }
        // the previous round ended with a synchronisation of this stream: its copy of h_guess has landed
        for (int s = 0; s < m; ++s) memcpy(V.h_guess[s].v, guesses ? guesses + (size_t)16 * (k + s) : kIdentityPose, sizeof(Pose16));
        SEQC(E, hipMemcpyAsync(V.d_guess, V.h_guess.get(), (size_t)m * sizeof(Pose16), hipMemcpyHostToDevice, E->stream));
        seq_enqueue_schedule(E, E->p.n_pyr - 1, false, nullptr, method, live);
        SEQC(E, hipGetLastError());
        const int rc = seq_finish_round(E, m, nullptr, method, live);
        if (rc) return rc;
        for (int s = 0; s < m; ++s)
            result_from_state(E->h_states[s], E->p.n_pyr, 0, poses_out + (size_t)16 * (k + s), results_out ? &results_out[k + s] : nullptr);
    }
    return 0;
}

}  // namespace

extern "C" {

int rgbd360_store_create(rgbd360_ctx* ctx, int capacity, int rows, int cols, rgbd360_store** out) {
    if (!out) return -1;
    *out = nullptr;
    if (!ctx) return -1;
    if (capacity < 1 || capacity > (1 << 20)) return fail(ctx, -1, "store capacity must be in 1..2^20");
    rgbd360_store* st = new rgbd360_store();
    st->ctx = ctx; st->p = ctx->p; st->capacity = capacity; st->rows = rows; st->cols = cols;
    st->max_eval_blocks = ctx->max_eval_blocks;
    std::string err;
    int rc = seq_create(st->p, std::min(capacity, kMaxSlots), rows, cols, st->max_eval_blocks, &st->put_eng, &err, kSeqPlanes);
    if (rc) {
        store_free(st);
        return fail(ctx, rc, err.c_str());
    }
    st->entries.resize(st->p.n_pyr);
    st->view.levels.resize(st->p.n_pyr);
    for (int l = 0; l < st->p.n_pyr; ++l) {
        const SeqLevel& L = st->put_eng->levels[l];
        rgbd360_store::Entries& A = st->entries[l];
        const size_t src_px = L.compact ? sizeof(float2) : sizeof(float4);
        const size_t np = (size_t)capacity * (size_t)L.n;
        if (A.src.ensure(np * (src_px / sizeof(float2))) != hipSuccess || A.trgP.ensure(np) != hipSuccess || A.trgD.ensure(np) != hipSuccess) {
            (void)hipGetLastError();
            store_free(st);
            return fail(ctx, -103, "out of device memory for the frame store");
        }
        st->view.levels[l] = StoreLevelView{reinterpret_cast<float4*>(A.src.get()), A.trgP, A.trgD};
        st->entry_bytes += (size_t)L.n * (src_px + 2 * sizeof(F3));
    }
    st->occupied.assign(capacity, 0);
    *out = st;
    return 0;
}

void rgbd360_store_destroy(rgbd360_store* st) { store_free(st); }

const char* rgbd360_store_last_error(rgbd360_store* st) { return st ? st->err.c_str() : "null store"; }

size_t rgbd360_store_entry_bytes(const rgbd360_store* st) { return st ? st->entry_bytes : 0; }

int rgbd360_store_occupied(const rgbd360_store* st, int entry) {
    if (!st || entry < 0 || entry >= st->capacity) return -1;
    return st->occupied[entry] ? 1 : 0;
}

int rgbd360_store_put(rgbd360_store* st, int n, const int* entry, const uint8_t* const* rgb, size_t rgb_step, const void* const* depth,
                      size_t depth_step, int depth_type, int on_device) {
    if (!st) return -1;
    if (n < 0) return store_fail(st, -1, "n must be >= 0");
    if (n == 0) return 0;
    if (!entry || !rgb || !depth) return store_fail(st, -1, "null pointer");
    if (depth_type != 0 && depth_type != 1) return store_fail(st, -1, "depth_type must be 0 (u16 mm) or 1 (f32 m)");
    const size_t dpx = depth_type == 0 ? 2 : 4;
    if (rgb_step < (size_t)st->cols * 3 || depth_step < (size_t)st->cols * dpx) return store_fail(st, -1, "row step smaller than a row");
    {
        std::vector<char> seen(st->capacity, 0);
        for (int k = 0; k < n; ++k) {
            if (entry[k] < 0 || entry[k] >= st->capacity)
                return store_fail(st, -1, "frame " + std::to_string(k) + ": entry " + std::to_string(entry[k]) + " is outside the store");
            if (seen[entry[k]]) return store_fail(st, -1, "frame " + std::to_string(k) + ": entry " + std::to_string(entry[k]) + " is named twice");
            seen[entry[k]] = 1;
            if (!rgb[k] || !depth[k]) return store_fail(st, -1, "null frame pointer");
        }
    }
    SeqEngine* E = st->put_eng;
    hipSetDevice(st->p.device);
    auto run = [&]() -> int {
        if (!on_device) {
            const int rc = seq_ensure_stage(E, depth_type);
            if (rc) return rc;
        }
        for (int k = 0; k < n; k += E->P) {
            const int m = std::min(E->P, n - k);
            const unsigned long long live = (1ull << m) - 1;      // m <= 32
            FramePtrs fp;
            EntryTable et;
            memset(&fp, 0, sizeof(fp));
            memset(&et, 0, sizeof(et));
            for (int s = 0; s < m; ++s) {
                et.e[s] = entry[k + s];
                if (on_device) {
                    fp.rgb[s] = rgb[k + s];
                    fp.depth[s] = depth[k + s];
                } else {      // stream-ordered behind the set-up launches that read the staging before
                    fp.rgb[s] = E->ring.rgb[0] + s * E->frame_bytes(3);
                    fp.depth[s] = E->ring.depth[0] + s * E->frame_bytes(dpx);
                    SEQC(E, copy_frame_h2d((uint8_t*)fp.rgb[s], (void*)fp.depth[s], rgb[k + s], rgb_step, depth[k + s], depth_step, depth_type, st->rows,
                                           st->cols, E->stream));
                }
            }
            seq_frame_setup(E, fp, on_device ? rgb_step : (size_t)st->cols * 3, on_device ? depth_step : (size_t)st->cols * dpx, depth_type, live, live,
                            live, 0, &st->view, &et);
            SEQC(E, hipGetLastError());
        }
        SEQC(E, hipStreamSynchronize(E->stream));      // the caller's images are free, and every engine's stream may read the entries
        return 0;
    };
    const int rc = run();
    if (rc) (void)hipStreamSynchronize(E->stream);
    for (int k = 0; k < n; ++k) st->occupied[entry[k]] = rc == 0;      // a failed put leaves its entries empty, not half written
    return rc ? store_fail(st, rc, E->err) : 0;
}

int rgbd360_store_align(rgbd360_store* st, int n_pairs, const int* trg, const int* src, const float* guesses, int method, int occlusion,
                        int n_inflight, float* poses_out, rgbd360_result* results_out) {
    if (!st) return -1;
    if (n_pairs < 0) return store_fail(st, -1, "n_pairs must be >= 0");
    if (n_inflight < 1 || n_inflight > 64) return store_fail(st, -1, "n_inflight must be in 1..64");
    if (method < 0 || method > 2) return store_fail(st, -4, "bad method");
    if (occlusion != 0) return store_fail(st, -1, "the frame store aligns with occlusion 0 only (the z-buffer passes have no slot dimension)");
    if (n_pairs == 0) return 0;
    if (!trg || !src || !poses_out) return store_fail(st, -1, "null pointer");
    for (int k = 0; k < n_pairs; ++k)      // checked here, all of them, before anything is launched: an index never reaches a kernel unchecked
        for (int role = 0; role < 2; ++role) {
            const int e = role == 0 ? trg[k] : src[k];
            const char* what = role == 0 ? "target" : "source";
            if (e < 0 || e >= st->capacity)
                return store_fail(st, -1, "pair " + std::to_string(k) + ": " + what + " entry " + std::to_string(e) + " is outside the store");
            if (!st->occupied[e])
                return store_fail(st, -1, "pair " + std::to_string(k) + ": " + what + " entry " + std::to_string(e) + " is empty");
        }
    hipSetDevice(st->p.device);
    // slots as rgbd360_align360_batch spreads them: two engines (own stream and host thread each) from 4 slots up
    const int S = std::min(n_inflight, n_pairs);
    const int n_eng = S >= 4 ? 2 : 1;
    const int P = (S + n_eng - 1) / n_eng;
    int rc = store_ensure_engines(st, n_eng, P);
    if (rc) return rc;
    int cnt[2] = {0, 0}, lo[2] = {0, 0}, hi[2] = {0, 0};
    for (int e = 0, o = 0; e < n_eng; ++e) {      // engine e: slots in proportion, a contiguous share of the list in proportion to its slots
        cnt[e] = S / n_eng + (e < S % n_eng ? 1 : 0);
        lo[e] = o;
        hi[e] = e + 1 == n_eng ? n_pairs : o + (int)(((long long)n_pairs * cnt[e] + S - 1) / S);
        hi[e] = std::min(hi[e], n_pairs);
        o = hi[e];
        st->eng[e]->libm = st->ctx->index_libm;
    }
    int rcs[2] = {0, 0};
    auto run_engine = [&](int e) {
        if (hi[e] <= lo[e]) return;
        rcs[e] = store_run_engine(st->eng[e], cnt[e], lo[e], hi[e], trg, src, guesses, method, poses_out, results_out);
        if (rcs[e]) (void)hipStreamSynchronize(st->eng[e]->stream);
    };
    run_on_threads(n_eng, run_engine);
    for (int e = 0; e < n_eng; ++e)
        if (rcs[e]) return store_fail(st, rcs[e], st->eng[e]->err);
    return 0;
}

}  // extern "C"
