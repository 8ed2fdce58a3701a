// map_align_plane_eval_tile.h -- the body of a point-to-plane evaluation kernel, included INSIDE k_vmap_plane_eval (map_align_plane.h) and
// k_vmap_plane_eval_batch (map_align_batch.h): one workgroup's tile of a source at a pose into one partial row.  One text for both kernels
// (see map_align_eval_tile.h).  No include guard.  The including kernel provides, under these names:
//   P, src, bx, by, table, mask, min_count, max_dist2, min_support, max_flatness, s_red (LDS, [kThreads / 64][kPlaneWords]), part_row(),
//   key3, d2_out, nr_out, class_out (per-point outputs or null), and SRC.
    float x[kPerThread], y[kPerThread], z[kPerThread];
    bool in[kPerThread];
    long long index[kPerThread];
    load_points<SRC>(src, bx, by, x, y, z, in, index);

    double acc[kPlRR + 2];           // n, H (21), g (6), r r, e.e; the counters are integers until the reduction
#pragma unroll
    for (int q = 0; q < kPlRR + 2; ++q) acc[q] = 0.0;
    unsigned n_probes = 0, n_valid = 0, n_box = 0, n_range = 0, n_unsupported = 0, n_nonplanar = 0, n_searched = 0;
    // one point after another through the one accumulator
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        if (!in[k]) continue;
        unsigned long long key = 0;
        long long f[3];
        float w[3];
        const int cls = classify(P, x[k], y[k], z[k], key, f, w);
        n_valid += cls >= 1 ? 1u : 0u;
        n_box += cls == 1 ? 1u : 0u;
        n_range += cls == 2 ? 1u : 0u;
        Match<PlaneSupport> mt;
        if (cls == 3) {
            n_searched += 1u;
            mt = search27<PlaneSupport>(table, mask, min_count, key, w, n_probes);
        }
        const bool kept = mt.best_key != kEmpty && mt.best <= max_dist2;
        const PlaneSupport& sp = mt.support;
        int pclass = kClassNone;
        double nrm[3] = {0.0, 0.0, 0.0}, r = 0.0;
        if (kept && sp.m < min_support) {
            pclass = kClassUnsupported;
            n_unsupported += 1u;
        } else if (kept) {
            const double dm = (double)sp.m;
            const double mx = sp.se[0] / dm, my = sp.se[1] / dm, mz = sp.se[2] / dm;
            const double cov[6] = {sp.see[0] / dm - mx * mx, sp.see[1] / dm - mx * my, sp.see[2] / dm - mx * mz,
                                   sp.see[3] / dm - my * my, sp.see[4] / dm - my * mz, sp.see[5] / dm - mz * mz};
            double l0, l1;
            if (plane_fit(cov, max_flatness, nrm, l0, l1)) {
                pclass = kClassKept;
                r = (nrm[0] * mx + nrm[1] * my) + nrm[2] * mz;
                const double wx = w[0], wy = w[1], wz = w[2];
                const double J[6] = {nrm[0], nrm[1], nrm[2], wy * nrm[2] - wz * nrm[1], wz * nrm[0] - wx * nrm[2], wx * nrm[1] - wy * nrm[0]};
                const double ex = mt.be[0], ey = mt.be[1], ez = mt.be[2];
                acc[kPlN] += 1.0;
                int h = kPlH;
#pragma unroll
                for (int a = 0; a < 6; ++a) {
#pragma unroll
                    for (int b = a; b < 6; ++b) acc[h++] += J[a] * J[b];
                }
#pragma unroll
                for (int a = 0; a < 6; ++a) acc[kPlG + a] += J[a] * r;
                acc[kPlRR] += r * r;
                acc[kPlEE] += (ex * ex + ey * ey) + ez * ez;
            } else {
                pclass = kClassNonplanar;
                n_nonplanar += 1u;
                nrm[0] = nrm[1] = nrm[2] = 0.0;
            }
        }
        if (key3) store_key3(key3 + 3 * index[k], mt.best_key, kept);
        if (d2_out) d2_out[index[k]] = mt.best;
        if (nr_out) {
            nr_out[4 * index[k]] = nrm[0];
            nr_out[4 * index[k] + 1] = nrm[1];
            nr_out[4 * index[k] + 2] = nrm[2];
            nr_out[4 * index[k] + 3] = r;
        }
        if (class_out) class_out[index[k]] = (uint8_t)pclass;
    }

    double row[kPlaneWords];
#pragma unroll
    for (int q = 0; q < kPlRR + 2; ++q) row[q] = acc[q];
    row[kPlValid] = (double)n_valid;
    row[kPlBox] = (double)n_box;
    row[kPlRange] = (double)n_range;
    row[kPlUnsupported] = (double)n_unsupported;
    row[kPlNonplanar] = (double)n_nonplanar;
    row[kPlProbes] = (double)n_probes;
    row[kPlSearched] = (double)n_searched;
    block_row_sum<kPlaneWords>(row, s_red, part_row());
