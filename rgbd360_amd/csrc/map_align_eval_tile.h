// map_align_eval_tile.h -- the body of a point-to-point evaluation kernel, included INSIDE k_vmap_icp_eval (map_align.h) and
// k_vmap_icp_eval_batch (map_align_batch.h): one workgroup's tile of a source at a pose into one partial row.  One text, so that a tile
// gives the same row in both kernels, and the single kernel's machine code is what it was before the batch kernel existed (an inlined
// function changed its schedule).  No include guard.  The including kernel provides, under these names:
//   P (vmap::Params with the pose), src (vmap::Source), bx, by (the tile and image row: load_points), table, mask, min_count, max_dist2,
//   s_red (LDS, [kThreads / 64][kIcpWords]), part_row() (the row to write, asked for once, at the end), key3, d2_out (per-point outputs or null), and SRC.
    float x[kPerThread], y[kPerThread], z[kPerThread];
    bool in[kPerThread];
    long long index[kPerThread];
    load_points<SRC>(src, bx, by, x, y, z, in, index);

    double acc[kIcpWords];
#pragma unroll
    for (int q = 0; q < kIcpWords; ++q) acc[q] = 0.0;
    unsigned n_probes = 0;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        if (!in[k]) continue;
        unsigned long long key = 0;
        long long f[3];
        float w[3];
        const int cls = classify(P, x[k], y[k], z[k], key, f, w);
        acc[17] += cls >= 1 ? 1.0 : 0.0;
        acc[18] += cls == 1 ? 1.0 : 0.0;
        acc[19] += cls == 2 ? 1.0 : 0.0;
        Match<NoSupport> mt;
        if (cls == 3) {
            acc[21] += 1.0;
            mt = search27<NoSupport>(table, mask, min_count, key, w, n_probes);
        }
        const bool kept = mt.best_key != kEmpty && mt.best <= max_dist2;
        if (key3) store_key3(key3 + 3 * index[k], mt.best_key, kept);
        if (d2_out) d2_out[index[k]] = mt.best;
        if (kept) {
            const double wx = w[0], wy = w[1], wz = w[2], ex = mt.be[0], ey = mt.be[1], ez = mt.be[2];
            acc[0] += 1.0;
            acc[1] += wx;
            acc[2] += wy;
            acc[3] += wz;
            acc[4] += wx * wx;
            acc[5] += wx * wy;
            acc[6] += wx * wz;
            acc[7] += wy * wy;
            acc[8] += wy * wz;
            acc[9] += wz * wz;
            acc[10] += ex;
            acc[11] += ey;
            acc[12] += ez;
            acc[13] += wy * ez - wz * ey;
            acc[14] += wz * ex - wx * ez;
            acc[15] += wx * ey - wy * ex;
            acc[16] += (ex * ex + ey * ey) + ez * ez;
        }
    }
    acc[20] = (double)n_probes;

    block_row_sum<kIcpWords>(acc, s_red, part_row());
