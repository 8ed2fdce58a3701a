// overlap_host_check.cpp -- the host side of the sensed-space overlap (rgbd360_overlap_candidates / rgbd360_overlap_representative,
// rgbd360_amd/csrc/rgbd360_host.cpp) as a program of its own, no device and no library, for a sanitizer build:
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/overlap_host_check.cpp -o overlap_host_check && ./overlap_host_check
// Walks the argument checks, empty and one-frame matrices, output truncation (max_out 0 and short), NULL outputs, every filter and the
// tie rules on seeded random matrices against a direct restatement.  Prints "ok" and returns 0, or the line of the first failure.
#include "../rgbd360_amd/csrc/rgbd360_host.cpp"

#include <random>

#define CHECK(c)                                                \
    do {                                                        \
        if (!(c)) {                                             \
            printf("failed at line %d: %s\n", __LINE__, #c);    \
            return 1;                                           \
        }                                                       \
    } while (0)

int main() {
    CHECK(rgbd360_overlap_candidates(-1, nullptr, 1, 0.f, 1, 0, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == -1);
    CHECK(rgbd360_overlap_candidates(2, nullptr, 1, 0.f, 1, 0, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == -1);
    CHECK(rgbd360_overlap_candidates(0, nullptr, 1, 0.f, 1, 0, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == 0);
    rgbd360_overlap one[1] = {};
    CHECK(rgbd360_overlap_candidates(1, one, 0, 0.f, 1, 0, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == -1);
    CHECK(rgbd360_overlap_candidates(1, one, 4, 0.f, 1, 0, 1, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == -1);
    CHECK(rgbd360_overlap_candidates(1, one, 4, 0.f, 1, 0, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == 0);
    const int sub0[1] = {0}, bad[2] = {0, 1};
    CHECK(rgbd360_overlap_representative(1, one, 4, sub0, 1) == 0);
    CHECK(rgbd360_overlap_representative(1, one, 4, bad, 2) == -1);
    CHECK(rgbd360_overlap_representative(1, one, 4, sub0, 0) == -1);
    CHECK(rgbd360_overlap_representative(0, one, 4, sub0, 1) == -1);

    std::mt19937 rng(7);
    for (int round = 0; round < 200; ++round) {
        const int n = 1 + (int)(rng() % 12), px = 64;
        std::vector<rgbd360_overlap> m((size_t)n * n);
        for (int a = 0; a < n; ++a)
            for (int b = 0; b < n; ++b) {
                rgbd360_overlap& r = m[(size_t)a * n + b];
                r = rgbd360_overlap();
                r.evaluated = a != b && rng() % 5 != 0;
                r.n_consistent = (int)(rng() % 9) * 8;      // few distinct values: ties
            }
        const float min_score = (float)(rng() % 5) / 8.f;
        const int min_gap = 1 + (int)(rng() % 3), per = (int)(rng() % 4), n_known = (int)(rng() % 4);
        std::vector<int> ka(n_known), kb(n_known);
        for (int k = 0; k < n_known; ++k) { ka[k] = (int)(rng() % n); kb[k] = (int)(rng() % n); }
        // restated: per b the qualifying a by (score descending, a ascending)
        std::vector<int> wa, wb;
        std::vector<float> ws;
        for (int b = 0; b < n; ++b) {
            std::vector<std::pair<float, int>> c;
            for (int a = 0; a + min_gap <= b; ++a) {
                const rgbd360_overlap &x = m[(size_t)a * n + b], &y = m[(size_t)b * n + a];
                const float s = x.evaluated && y.evaluated ? (float)std::min(x.n_consistent, y.n_consistent) / (float)px : 0.f;
                bool known = false;
                for (int k = 0; k < n_known; ++k) known = known || (ka[k] == a && kb[k] == b) || (ka[k] == b && kb[k] == a);
                if (s >= min_score && !known) c.push_back({-s, a});
            }
            std::sort(c.begin(), c.end());
            if (per > 0 && (int)c.size() > per) c.resize(per);
            for (const auto& e : c) { wa.push_back(e.second); wb.push_back(b); ws.push_back(-e.first); }
        }
        const int cap = (int)wa.size();
        for (int max_out : {cap, cap / 2, 0}) {
            std::vector<int> oa(max_out), ob(max_out);      // exactly max_out long: a write past it is a sanitizer report
            std::vector<float> os(max_out);
            const int found = rgbd360_overlap_candidates(n, m.data(), px, min_score, min_gap, per, n_known, ka.data(), kb.data(), max_out, oa.data(),
                                                         ob.data(), os.data());
            CHECK(found == cap);
            for (int k = 0; k < max_out; ++k) CHECK(oa[k] == wa[k] && ob[k] == wb[k] && os[k] == ws[k]);
        }
        CHECK(rgbd360_overlap_candidates(n, m.data(), px, min_score, min_gap, per, n_known, ka.data(), kb.data(), cap, nullptr, nullptr, nullptr) == cap);
        std::vector<int> sub;
        for (int a = 0; a < n; ++a)
            if (rng() % 2) sub.push_back(a);
        if (sub.empty()) sub.push_back((int)(rng() % n));
        std::shuffle(sub.begin(), sub.end(), rng);
        int best = sub[0];
        double best_sum = -1.0;
        for (int u : sub) {
            double sum = 0.0;
            for (int v : sub) {
                if (u == v) continue;
                const rgbd360_overlap &x = m[(size_t)u * n + v], &y = m[(size_t)v * n + u];
                sum += x.evaluated && y.evaluated ? (double)((float)std::min(x.n_consistent, y.n_consistent) / (float)px) : 0.0;
            }
            if (sum > best_sum) { best_sum = sum; best = u; }
        }
        CHECK(rgbd360_overlap_representative(n, m.data(), px, sub.data(), (int)sub.size()) == best);
    }
    printf("ok\n");
    return 0;
}
