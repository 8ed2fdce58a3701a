// map_align_solve_rows.h -- the body of a solve kernel, included INSIDE k_vmap_icp_solve<M> (map_align.h) and k_vmap_icp_solve_batch<M>
// (map_align_batch.h): the partial rows of one alignment added in ascending order, then lane 0's step.  One text for both kernels (see
// map_align_eval_tile.h).  No include guard.  The including kernel provides, under these names: st (LoopState<M::kWords>*), trace, part,
// n_rows, final_pass, min_matches, eps, s_row (LDS, [M::kWords]) and M.
    const int t = threadIdx.x;
    if (t < M::kWords) {         // the rows in ascending order
        double s = 0.0;
        for (int r = 0; r < n_rows; ++r) s += part[(size_t)r * M::kWords + t];
        s_row[t] = s;
        st->row[t] = s;
    }
    __syncthreads();
    if (t != 0) return;
    const long long n = (long long)s_row[M::kN];
    if (final_pass) {
        M::assemble(s_row, st->H, st->g);
        if (st->status == RGBD360_OK && n < min_matches) st->status = RGBD360_NO_VALID_PIXELS;
        st->done = 1;
        return;
    }
    if (n < min_matches) {
        st->status = RGBD360_NO_VALID_PIXELS;
        st->done = 1;
        return;
    }
    float H[36], g[6], pose[16], pose_new[16], u[6];
    M::assemble(s_row, H, g);
    for (int k = 0; k < 16; ++k) pose[k] = st->pose[k];
    if (gn::step(H, g, 0.f, pose, pose_new, u) != 0) {
        st->status = RGBD360_ILL_POSED;
        st->done = 1;
        return;
    }
    for (int k = 0; k < 16; ++k) st->pose[k] = pose_new[k];
    rgbd360_map_align_trace rec;
    rec.n = n;
    rec.sum_sq = s_row[M::kSumSq];
    for (int k = 0; k < 6; ++k) rec.update[k] = u[k];
    trace[st->iterations] = rec;
    st->iterations += 1;
    const float vv = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2], ww = (u[3] * u[3] + u[4] * u[4]) + u[5] * u[5];
    if (vv <= eps && ww <= eps) {
        st->converged = 1;
        st->done = 1;
    }
