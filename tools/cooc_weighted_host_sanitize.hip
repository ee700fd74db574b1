// The host walk of the weighted neighbours of items (sml_cooc_weighted_host_walk in knn.hip) under the host sanitizers, as a
// stand-alone program: it includes the source and runs the walk over heap arrays sized exactly (so a read or write one element
// out of place is an AddressSanitizer report) with users whose weights are junk (+0, negative, NaN, inf, out of the fixed point's
// range, rounding to 0), an item with no user (an empty row), a repeated `rows` entry, norms and a filter, and checks identity (a)
// of the header against sml_cooc_host_walk on the way.  It starts no kernel and needs no GPU.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/cooc_weighted_host_sanitize.hip -o cooc_weighted_host_sanitize && ./cooc_weighted_host_sanitize
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../sml_amd/csrc/knn.hip"

static uint32_t rnd_state = 2500u;
static uint32_t rnd() { return rnd_state = rnd_state * 1664525u + 1013904223u; }

static int run(int F, int k) {
    const int64_t n_user = 37, n_item = 101;                 // item 100 has no user; user 0 has no item; user 1 holds items 0 .. 99
    std::vector<std::vector<int32_t>> sets(n_user);
    for (int32_t i = 0; i < n_item - 1; ++i) sets[1].push_back(i);
    for (int64_t u = 2; u < n_user; ++u)
        for (int32_t i = 0; i < n_item - 1; ++i)
            if (rnd() % 100 < (uint32_t)(3 + u % 17)) sets[u].push_back(i);
    std::vector<int64_t> u_off(n_user + 1, 0), i_off(n_item + 1, 0);
    std::vector<int32_t> u_items, i_users;
    for (int64_t u = 0; u < n_user; ++u) {
        u_items.insert(u_items.end(), sets[u].begin(), sets[u].end());
        u_off[u + 1] = (int64_t)u_items.size();
    }
    for (int32_t i = 0; i < n_item; ++i) {
        for (int64_t u = 0; u < n_user; ++u)
            for (const int32_t j : sets[u])
                if (j == i) i_users.push_back((int32_t)u);
        i_off[i + 1] = (int64_t)i_users.size();
    }
    std::vector<float> w(n_user);
    for (int64_t u = 0; u < n_user; ++u) w[u] = sets[u].empty() ? 0.0f : 1.0f / (float)sets[u].size();
    const float s = std::ldexp(1.0f, -F);
    w[1] = 0.125f;
    w[5] = 0.0f; w[6] = -1.0f; w[7] = NAN; w[8] = INFINITY;   // contribute nothing
    w[9] = std::ldexp(s, 33);                                  // 2^33 in fixed point: out of range
    w[10] = std::ldexp(s, 32);                                 // 2^32: the last value in range
    w[11] = 0.25f * s;                                         // rounds to 0
    w[12] = 0.5f * s; w[13] = 1.5f * s; w[14] = 2.5f * s;     // ties to even: 0, 2, 2
    std::vector<double> na(n_item), nb(n_item);
    for (int32_t i = 0; i < n_item; ++i) {
        const double deg = (double)(i_off[i + 1] - i_off[i]);
        na[i] = deg;
        nb[i] = std::pow(deg, 0.6);
    }
    std::vector<uint32_t> allow((n_item + 31) / 32);
    for (auto& v : allow) v = rnd() | rnd();
    std::vector<int64_t> rows = {3, 100, 0, 3, 99, 57};      // row 3 twice; item 100 is the empty row
    const int64_t n = (int64_t)rows.size();
    for (int pass = 0; pass < 3; ++pass) {
        // pass 0: no norms, no filter, named rows; pass 1: norms, shrink and filter; pass 2: rows == NULL, every row
        const int64_t m = pass == 2 ? n_item : n;
        std::vector<int32_t> items((size_t)m * k, 77), ne((size_t)m, 77);
        std::vector<float> sims((size_t)m * k, 7.0f);
        const SmlCoocWeighted a = {i_off.data(), i_users.data(), u_off.data(), u_items.data(), n_user, n_item, pass == 2 ? nullptr : rows.data(),
                                   m, w.data(), F, pass ? na.data() : nullptr, pass ? nb.data() : nullptr, pass == 1 ? 10.0 : 0.0,
                                   pass == 1 ? allow.data() : nullptr, k};
        sml_cooc_weighted_host_walk(a, items.data(), sims.data(), ne.data());
        const int64_t empty = pass == 2 ? 100 : 1;           // where item 100's row is written
        if (ne[empty] != 0 || items[empty * k] != -1 || sims[empty * k] != -INFINITY) return 1 + pass * 10;
        // the row named twice (outputs 0 and 3 of the named rows) is written twice with the same bytes
        if (pass != 2 && (std::memcmp(&items[0], &items[3 * k], 4 * k) != 0 || std::memcmp(&sims[0], &sims[3 * k], 4 * k) != 0 || ne[0] != ne[3]))
            return 2 + pass * 10;
        for (int64_t x = 0; x < m; ++x)
            for (int q = 0; q < k; ++q) {
                const int32_t j = items[x * k + q];
                if (j < -1 || j >= n_item || (j == -1) != (q >= ne[x] || q >= k) || (j >= 0 && !(sims[x * k + q] > 0.0f))) return 3 + pass * 10;
            }
    }
    // identity (a): unit weights at F = 0 return the unweighted walk's bytes at min_co = 1
    std::vector<float> ones(n_user, 1.0f);
    std::vector<int32_t> it_w((size_t)n_item * k), it_c((size_t)n_item * k), ne_w(n_item), ne_c(n_item);
    std::vector<float> s_w((size_t)n_item * k), s_c((size_t)n_item * k);
    const SmlCoocWeighted aw = {i_off.data(), i_users.data(), u_off.data(), u_items.data(), n_user, n_item, nullptr, n_item, ones.data(), 0,
                                na.data(), nb.data(), 1.0, nullptr, k};
    const SmlCooc ac = {i_off.data(), i_users.data(), u_off.data(), u_items.data(), n_user, n_item, nullptr, n_item, na.data(), nb.data(), 1.0,
                        1, nullptr, k};
    sml_cooc_weighted_host_walk(aw, it_w.data(), s_w.data(), ne_w.data());
    sml_cooc_host_walk(ac, it_c.data(), s_c.data(), ne_c.data());
    if (std::memcmp(it_w.data(), it_c.data(), it_w.size() * 4) != 0 || std::memcmp(s_w.data(), s_c.data(), s_w.size() * 4) != 0 ||
        std::memcmp(ne_w.data(), ne_c.data(), ne_w.size() * 4) != 0)
        return 40;
    return 0;
}

int main() {
    int rc = 0;
    for (const int F : {0, 30, 32})
        for (const int k : {1, 5, 128})
            rc = rc ? rc : run(F, k);
    std::printf(rc ? "weighted co-occurrence host walk: FAILED (%d)\n" : "weighted co-occurrence host walk: clean (%d)\n", rc);
    return rc;
}
