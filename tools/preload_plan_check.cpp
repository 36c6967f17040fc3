// Stand-alone check of the host side of the preload crop (csrc/preload.hip), meant for a sanitizer build of the HOST code (no
// GPU is touched: the planner makes no HIP call and the launch entries are only given arguments they must refuse, or empty
// calls that launch nothing):
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         open3dsot_amd/csrc/preload.hip tools/preload_plan_check.cpp -o preload_plan_check && ./preload_plan_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/o3dsot.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
    const int sizes[] = {0, 1, 255, 256, 257, 1000, 120000};
    alignas(16) static float word[4];
    int32_t* iw = reinterpret_cast<int32_t*>(word);
    for (int F : {1, 2, 7, 100, O3D_PRELOAD_MAX_FRAMES}) {
        std::vector<int32_t> t(6 * (size_t)F, -1);          // exactly F records: a read or write past the table is caught
        long row = 0;
        for (int f = 0; f < F; ++f) {
            t[6 * f] = (int32_t)row; t[6 * f + 1] = sizes[f % 7]; t[6 * f + 3] = (f * 37) % 67;      // 0..66 boxes: record 0 has none
            row += sizes[f % 7];
        }
        int grid[2] = {-1, -1};
        const long got = o3d_preload_scratch(t.data(), F, row, grid);
        long wgs = 0, boxes = 0, need = 0;
        for (int f = 0; f < F; ++f) {
            CHECK(t[6 * f + 2] == boxes && t[6 * f + 4] == wgs && t[6 * f + 5] == need);
            const long n = t[6 * f + 1], nb = t[6 * f + 3];
            const long W = nb == 0 ? 0 : n > 0 ? (n + 255) / 256 : 1;
            wgs += W; boxes += nb; need += W * nb;
        }
        CHECK(got == need && grid[0] == wgs && grid[1] == boxes);
        CHECK(o3d_preload_scratch(t.data(), F, row, nullptr) == need);
        const int B = (int)boxes;
        // refused before any HIP call: no device table, no scratch, a short scratch, a wrong B, rows short, an edited plan
        CHECK(o3d_preload_count(word, row, t.data(), nullptr, F, word, B, nullptr, iw, need, iw, nullptr) == (B ? O3D_EINVAL : O3D_OK));
        if (B == 0) continue;
        CHECK(o3d_preload_count(word, row, t.data(), iw, F, word, B, nullptr, nullptr, need, iw, nullptr) == O3D_EINVAL);
        CHECK(o3d_preload_count(word, row, t.data(), iw, F, word, B, nullptr, iw, need - 1, iw, nullptr) == O3D_EINVAL);
        CHECK(o3d_preload_count(word, row, t.data(), iw, F, word, B + 1, nullptr, iw, need, iw, nullptr) == O3D_EINVAL);
        CHECK(o3d_preload_count(word, row, t.data(), iw, F, word, B, nullptr, iw, need, nullptr, nullptr) == O3D_EINVAL);
        CHECK(o3d_preload_count(word + 1, row, t.data(), iw, F, word, B, nullptr, iw, need, iw, nullptr) == O3D_EINVAL);
        CHECK(o3d_preload_scatter(word, row, t.data(), iw, F, word, B, nullptr, iw, need, nullptr, word, 1, nullptr) == O3D_EINVAL);
        CHECK(o3d_preload_scatter(word, row, t.data(), iw, F, word, B, nullptr, iw, need, (const long*)word, nullptr, 1, nullptr) == O3D_EINVAL);
        CHECK(o3d_preload_scatter(word, row, t.data(), iw, F, word, B, nullptr, iw, need, (const long*)word, word, -1, nullptr) == O3D_EINVAL);
        // the posed pair: the same refusals, and its own (row_floats, the poses)
        const double* dp = reinterpret_cast<const double*>(word);
        for (int rf : {3, 4}) {
            CHECK(o3d_preload_posed_count(word, row, rf, t.data(), nullptr, F, word, B, dp, iw, need, iw, nullptr) == O3D_EINVAL);
            CHECK(o3d_preload_posed_count(word, row, rf, t.data(), iw, F, word, B, dp, iw, need - 1, iw, nullptr) == O3D_EINVAL);
            CHECK(o3d_preload_posed_count(word, row, rf, t.data(), iw, F, word, B + 1, dp, iw, need, iw, nullptr) == O3D_EINVAL);
            CHECK(o3d_preload_posed_count(word, row, rf, t.data(), iw, F, word, B, nullptr, iw, need, iw, nullptr) == O3D_EINVAL);
            CHECK(o3d_preload_posed_count(word, row, rf, t.data(), iw, F, word, B, (const double*)(word + 1), iw, need, iw, nullptr) == O3D_EINVAL);
            CHECK(o3d_preload_posed_scatter(word, row, rf, t.data(), iw, F, word, B, dp, iw, need, nullptr, word, 1, nullptr) == O3D_EINVAL);
            CHECK(o3d_preload_posed_scatter(word, row, rf, t.data(), iw, F, word, B, dp, iw, need, (const long*)word, word, -1, nullptr) == O3D_EINVAL);
            CHECK(o3d_preload_posed_scatter(word, row, rf, t.data(), iw, F, word, B, nullptr, iw, need, (const long*)word, word, 1, nullptr) == O3D_EINVAL);
        }
        CHECK(o3d_preload_posed_count(word + 1, row, 4, t.data(), iw, F, word, B, dp, iw, need, iw, nullptr) == O3D_EINVAL);
        for (int rf : {-1, 0, 2, 5})
            CHECK(o3d_preload_posed_count(word, row, rf, t.data(), iw, F, word, B, dp, iw, need, iw, nullptr) == O3D_EINVAL);
        if (row > 0) CHECK(o3d_preload_count(word, row - 1, t.data(), iw, F, word, B, nullptr, iw, need, iw, nullptr) == O3D_EINVAL);
        t[6 * (F - 1) + 5] += 1;
        CHECK(o3d_preload_count(word, row, t.data(), iw, F, word, B, nullptr, iw, need + 1, iw, nullptr) == O3D_EINVAL);
        t[6 * (F - 1) + 1] = -1;
        CHECK(o3d_preload_scratch(t.data(), F, row, grid) == -1);
    }
    std::vector<int32_t> one = {0, 3, 0, 1, 0, 0};
    CHECK(o3d_preload_scratch(nullptr, 1, 3, nullptr) == -1);
    CHECK(o3d_preload_scratch(nullptr, 0, 0, nullptr) == 0);
    CHECK(o3d_preload_scratch(one.data(), O3D_PRELOAD_MAX_FRAMES + 1, 3, nullptr) == -1);
    CHECK(o3d_preload_scratch(one.data(), 1, (long)O3D_PRELOAD_MAX_ROWS + 1, nullptr) == -1);
    CHECK(o3d_preload_scratch(one.data(), 1, 2, nullptr) == -1);
    one[3] = O3D_PRELOAD_MAX_BOXES + 1;
    CHECK(o3d_preload_scratch(one.data(), 1, 3, nullptr) == -1);
    CHECK(o3d_preload_count(nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr) == O3D_OK);
    CHECK(o3d_preload_scatter(nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr) == O3D_OK);
    CHECK(o3d_preload_posed_count(nullptr, 0, 3, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr) == O3D_OK);
    CHECK(o3d_preload_posed_scatter(nullptr, 0, 4, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr) == O3D_OK);
    CHECK(o3d_preload_posed_count(nullptr, 0, 2, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr) == O3D_EINVAL);
    std::printf("preload planner: ok\n");
    return 0;
}
