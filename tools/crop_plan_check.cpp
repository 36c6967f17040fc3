// Stand-alone check of the host planner of o3d_track_crop_groups (csrc/train_batch.hip), meant for a sanitizer build of the HOST
// code (no GPU is touched: the planner makes no HIP call and the launch entry is only given tables it must refuse):
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         open3dsot_amd/csrc/train_batch.hip tools/crop_plan_check.cpp -o crop_plan_check && ./crop_plan_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/o3dsot.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
    static float cloud[3];
    static o3d_crop_target targets[1];
    const int sizes[] = {0, 1, 255, 256, 257, 1000, 120000};
    for (int G : {1, 2, 7, 100, O3D_CROP_MAX_GROUPS}) {
        std::vector<o3d_crop_plan> plan(G);                 // exactly G records: a read or write past the table is caught
        long wgs = 0, rows = 0, need = 0;
        for (int g = 0; g < G; ++g) {
            plan[g] = o3d_crop_plan{cloud, sizes[g % 7], targets, 1 + (g * 37) % O3D_CROP_MULTI_MAX_TARGETS, -1, -1, -1};
        }
        int grid[2] = {-1, -1};
        const long got = o3d_track_crop_groups_scratch(plan.data(), G, grid);
        for (int g = 0; g < G; ++g) {
            CHECK(plan[g].wg_start == wgs && plan[g].row_start == rows && plan[g].sbase == need);
            const long W = plan[g].n > 0 ? (plan[g].n + 255) / 256 : 1;
            wgs += W; rows += plan[g].n_targets; need += W * plan[g].n_targets;
        }
        CHECK(got == need && grid[0] == wgs && grid[1] == rows);
        CHECK(o3d_track_crop_groups_scratch(plan.data(), G, nullptr) == need);
        // the launch entry refuses, before any HIP call: no device table, no scratch, a short scratch, a plan that was edited
        int32_t word = 0;
        CHECK(o3d_track_crop_groups(plan.data(), nullptr, G, &word, need, nullptr) == O3D_EINVAL);
        CHECK(o3d_track_crop_groups(plan.data(), plan.data(), G, nullptr, need, nullptr) == O3D_EINVAL);
        CHECK(o3d_track_crop_groups(plan.data(), plan.data(), G, &word, need - 1, nullptr) == O3D_EINVAL);
        plan[G - 1].sbase += 1;
        CHECK(o3d_track_crop_groups(plan.data(), plan.data(), G, &word, need + 1, nullptr) == O3D_EINVAL);
        plan[G - 1].n = -1;
        CHECK(o3d_track_crop_groups_scratch(plan.data(), G, grid) == -1);
    }
    std::vector<o3d_crop_plan> one(1, o3d_crop_plan{cloud, 3, targets, 1, 0, 0, 0});
    CHECK(o3d_track_crop_groups_scratch(nullptr, 1, nullptr) == -1);
    CHECK(o3d_track_crop_groups_scratch(one.data(), 0, nullptr) == -1);
    CHECK(o3d_track_crop_groups_scratch(one.data(), O3D_CROP_MAX_GROUPS + 1, nullptr) == -1);
    one[0].n_targets = O3D_CROP_MULTI_MAX_TARGETS + 1;
    CHECK(o3d_track_crop_groups_scratch(one.data(), 1, nullptr) == -1);
    std::printf("crop planner: ok\n");
    return 0;
}
