// The two host walks of the clustered index (sml_ivf_host_walk in retrieval.hip, sml_ivf_centroids_host_walk in ivf.hip) under the
// host sanitizers, as a stand-alone program: it includes the two sources, runs the walks over heap arrays sized exactly (so a
// read or write one element out of place is an AddressSanitizer report) with padding probes, a list probed twice, empty lists,
// Seen, a filter and score terms, at every (d, element type) pair, and exits 0.  It starts no kernel and needs no GPU.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/ivf_host_sanitize.hip -o ivf_host_sanitize && ./ivf_host_sanitize
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../sml_amd/csrc/retrieval.hip"
#include "../sml_amd/csrc/ivf.hip"

static uint32_t rnd_state = 12345u;
static uint32_t rnd() { return rnd_state = rnd_state * 1664525u + 1013904223u; }
static float rndf() { return (float)(rnd() >> 8) / (float)(1 << 24) - 0.5f; }

template <class T>
static int run(int d) {
    const int64_t n_item = 403, n_user = 9, n = 7;
    const int n_list = 13, nprobe = 5, k = 20;
    std::vector<T> wu(n_user * d), wi(n_item * d), cin(n_list * d), cout(n_list * d);
    for (auto& v : wu) v = (T)rndf();
    for (auto& v : wi) v = (T)rndf();
    for (auto& v : cin) v = (T)rndf();
    // lists: item i belongs to list (i * 7) % 11, so lists 11 and 12 are empty; ids ascend inside each list
    std::vector<int64_t> off(n_list + 1, 0);
    std::vector<int32_t> items;
    for (int c = 0; c < n_list; ++c) {
        for (int64_t i = 0; i < n_item; ++i)
            if ((i * 7) % 11 == c) items.push_back((int32_t)i);
        off[c + 1] = (int64_t)items.size();
    }
    if ((int64_t)items.size() != n_item) return 1;
    std::vector<int64_t> users = {3, 7, 3, 0, 8, 1, 5};
    std::vector<int32_t> probes(n * nprobe);
    for (auto& p : probes) p = (int32_t)(rnd() % (n_list + 6)) - 3;          // -3 .. n_list + 2: padding on both sides
    probes[0] = probes[1] = 4;                                               // a list probed twice
    probes[5] = 11; probes[6] = 12;                                          // the empty lists
    std::vector<int64_t> seen_off(n_user + 1, 0);
    std::vector<int32_t> seen_items;
    for (int64_t u = 0; u < n_user; ++u) {
        for (int64_t i = u; i < n_item; i += 5 + u) seen_items.push_back((int32_t)i);
        seen_off[u + 1] = (int64_t)seen_items.size();
    }
    const int64_t n_pad = (n_item + 31) / 32 * 32;
    std::vector<uint32_t> allow(n_pad / 32);
    for (auto& w : allow) w = rnd() | rnd();
    std::vector<float> adj(2 * n_pad);
    for (auto& v : adj) v = rndf();
    std::vector<int32_t> out_i(n * k), n_elig(n);
    std::vector<float> out_s(n * k);
    const SmlIvfLists l = {off.data(), items.data(), n_list, probes.data(), nprobe};
    for (int variant = 0; variant < 4; ++variant) {
        const SmlCatalogue c = {d, (int)sizeof(T), wu.data(), wi.data(), n_item, seen_off.data(), seen_items.data(),
                                (variant & 1) ? allow.data() : nullptr, (variant & 2) ? adj.data() : nullptr};
        if (!sml_ivf_host_walk(c, users.data(), n, l, k, out_i.data(), out_s.data(), n_elig.data())) return 2;
        for (int64_t x = 0; x < n; ++x)
            for (int q = 1; q < k; ++q)
                if (out_i[x * k + q] >= 0 && !(out_s[x * k + q - 1] >= out_s[x * k + q])) return 3;       // sorted, no NaN
    }
    if (!sml_ivf_centroids_host_walk(d, (int)sizeof(T), wi.data(), off.data(), items.data(), n_list, cin.data(), cout.data())) return 4;
    for (int s = 0; s < d; ++s)
        if ((float)cout[11 * d + s] != (float)cin[11 * d + s]) return 5;                                    // an empty list keeps its row
    if (!sml_ivf_centroids_host_walk(d, (int)sizeof(T), wi.data(), off.data(), items.data(), n_list, cin.data(), cin.data())) return 6;
    for (size_t q = 0; q < cin.size(); ++q)
        if ((float)cin[q] != (float)cout[q]) return 7;                                                      // in place = out of place
    return 0;
}

int main() {
    int rc = run<float>(32);
    rc = rc ? rc : run<float>(64);
    rc = rc ? rc : run<_Float16>(32);
    rc = rc ? rc : run<_Float16>(64);
    rc = rc ? rc : run<_Float16>(128);
    std::printf(rc ? "ivf host walks: FAILED (%d)\n" : "ivf host walks: clean (%d)\n", rc);
    return rc;
}
