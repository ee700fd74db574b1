// The two host walks of the fold-in (sml_gram_host_walk and sml_als_host_walk in als.hip) under the host sanitizers, as a
// stand-alone program: it includes the source, runs the walks over heap arrays sized exactly (so a read or write one element out
// of place is an AddressSanitizer report) with an empty row, a failing row, a repeated `rows` entry and n_rows off a chunk
// boundary, at every (d, element type) pair, and exits 0.  It starts no kernel and needs no GPU.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/als_host_sanitize.hip -o als_host_sanitize && ./als_host_sanitize
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../sml_amd/csrc/als.hip"

static uint32_t rnd_state = 2222u;
static uint32_t rnd() { return rnd_state = rnd_state * 1664525u + 1013904223u; }
static float rndf() { return (float)(rnd() >> 8) / (float)(1 << 24) - 0.5f; }

template <class T>
static int run(int d) {
    const int64_t n_other = 1027, n_out = 9;                 // 1027: one whole chunk and three rows
    std::vector<T> other(n_other * d), out(n_out * d);
    for (auto& v : other) v = (T)rndf();
    for (auto& v : out) v = (T)7.0f;
    for (int s = 0; s < d; ++s) other[5 * d + s] = (T)0.0f;  // row 5: all zero, the failing member with reg = alpha0 = 0
    std::vector<double> gram((size_t)d * d), gram1((size_t)d * d);
    if (!sml_gram_host_walk(d, (int)sizeof(T), other.data(), n_other, gram.data())) return 1;
    if (!sml_gram_host_walk(d, (int)sizeof(T), other.data(), 1, gram1.data())) return 2;
    for (int a = 0; a < d; ++a)
        for (int b = 0; b < d; ++b)
            if (std::memcmp(&gram[a * d + b], &gram[b * d + a], 8) != 0) return 3;                 // both triangles, bit for bit
    // sets of the 9 rows: row 2 is empty, row 4 holds only the zero row, row 8 the last row of the table, row 6 is heavy
    std::vector<int64_t> off(n_out + 1, 0);
    std::vector<int32_t> items;
    for (int64_t u = 0; u < n_out; ++u) {
        if (u == 4) items.push_back(5);
        else if (u == 8) items.push_back((int32_t)(n_other - 1));
        else if (u == 6) for (int64_t i = 0; i < n_other; i += 2) items.push_back((int32_t)i);
        else if (u != 2) for (int64_t i = u; i < n_other; i += 97 + u) items.push_back((int32_t)i);
        off[u + 1] = (int64_t)items.size();
    }
    std::vector<int64_t> rows = {3, 8, 2, 4, 3, 6, 0};       // row 3 twice; rows 1, 5, 7 are not named
    std::vector<int32_t> status(rows.size(), 77);
    if (!sml_als_host_walk(d, (int)sizeof(T), other.data(), gram.data(), 0.1, 0.1, off.data(), items.data(), rows.data(), (int64_t)rows.size(),
                           out.data(), status.data()))
        return 4;
    const int32_t want[] = {0, 0, 1, 0, 0, 0, 0};
    for (size_t x = 0; x < rows.size(); ++x)
        if (status[x] != want[x]) return 5;
    for (int s = 0; s < d; ++s) {
        if ((float)out[2 * d + s] != 0.0f) return 6;                                                 // the empty row is written as zero
        if ((float)out[1 * d + s] != 7.0f || (float)out[5 * d + s] != 7.0f || (float)out[7 * d + s] != 7.0f) return 7;   // not named
    }
    // reg = alpha0 = 0, no Gram: the zero member row cannot be solved and keeps its bytes; rows == NULL walks every row
    std::vector<T> out2(n_out * d);
    for (auto& v : out2) v = (T)7.0f;
    std::vector<int32_t> status2(n_out, 77);
    if (!sml_als_host_walk(d, (int)sizeof(T), other.data(), nullptr, 0.0, 0.0, off.data(), items.data(), nullptr, n_out, out2.data(),
                           status2.data()))
        return 8;
    if (status2[4] != 2 || status2[2] != 1) return 9;
    for (int s = 0; s < d; ++s)
        if ((float)out2[4 * d + s] != 7.0f) return 10;
    return 0;
}

int main() {
    int rc = run<float>(32);
    rc = rc ? rc : run<float>(64);
    rc = rc ? rc : run<_Float16>(32);
    rc = rc ? rc : run<_Float16>(64);
    std::printf(rc ? "als host walks: FAILED (%d)\n" : "als host walks: clean (%d)\n", rc);
    return rc;
}
