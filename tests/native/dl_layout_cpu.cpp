// Host build of the exact path's workspace layout (oflibnumpy_amd/csrc/ofl_delaunay_ws.h, the very header the stage files
// include) over a table of shapes.  Stand-alone: exits 0 and prints the number of layouts checked, or prints the first
// broken rule and exits 1.  tests/test_delaunay_layout_host.py builds it with -fsanitize=address,undefined.
//
// The totals are literals: what ofl_scatter_workspace_bytes reported for the shape, less the diagonal-plane tail that
// ofl_scatter.hip adds, when the layout was still 35 hand-aligned lines.  Callers size buffers from that number and the slab
// mode leaves state in a workspace between two calls, so a total that moves is a break of the ABI, not a detail.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "../../oflibnumpy_amd/csrc/ofl_delaunay_ws.h"

namespace {

using namespace ofl_dlw;

struct Shape { int H, W; size_t total; };

// pixel counts of every residue class that matters: 1, odd, 4 n off the 256-byte grid, on it, and the sizes of the benchmark
const Shape kShapes[] = {
    { 1, 1, 300800 },          { 5, 7, 306176 },             { 9, 33, 364544 },
    { 96, 128, 3048704 },      { 17, 4099, 15909888 },       { 300, 400, 27183104 },
    { 1080, 1920, 464907008 }, { 2160, 3840, 1858745344ull }, { 4320, 7680, 7434095616ull },
};

int broken(const Shape &s, const char *rule, const char *part = "")
{
    printf("%d x %d: %s %s\n", s.H, s.W, rule, part);
    return 1;
}

int check(const Shape &s, void *base)
{
    std::vector<DlPart> parts;
    size_t total = 0;
    const DlWs ws = carve_exact(base, s.H, s.W, &total, &parts);
    const size_t n = (size_t)s.H * s.W;
    if (parts.size() != 31) return broken(s, "the table does not have the 31 parts of DlWs");
    if (parts[0].offset != 0) return broken(s, "the first part does not start the workspace", parts[0].name);
    for (size_t i = 0; i < parts.size(); ++i) {
        const DlPart &p = parts[i];
        if (p.offset % 256) return broken(s, "part off the 256-byte grid:", p.name);
        // disjoint and in declaration order: the next part starts where this one's slot ends, the last slot ends at the total
        const size_t end = align_up(p.offset + p.bytes, 256);
        const size_t next = i + 1 < parts.size() ? parts[i + 1].offset : total;
        if (p.offset + p.bytes > next) return broken(s, "part runs into the next one:", p.name);
        if (end != next) return broken(s, i + 1 < parts.size() ? "gap or overlap after part" : "the last part does not end at the total:", p.name);
    }
    const DlPart &owner = parts.back();
    if (strcmp(owner.name, "owner") || owner.bytes != n * 4) return broken(s, "owner is not the last part, H * W words long");
    // the members point where the table says
    const uintptr_t b = reinterpret_cast<uintptr_t>(base);
    if (reinterpret_cast<uintptr_t>(ws.head) != b || reinterpret_cast<uintptr_t>(ws.owner) != b + owner.offset ||
        reinterpret_cast<uintptr_t>(ws.pool) != b + parts[24].offset || strcmp(parts[24].name, "pool"))
        return broken(s, "a member does not point at its part");
    if (ws.oy0 != 0 || ws.oy1 != s.H) return broken(s, "the owner map does not cover rows [0, H)");
    if (total != s.total) { printf("%d x %d: total %zu, recorded %zu\n", s.H, s.W, total, s.total); return 1; }
    return 0;
}

}  // namespace

int main()
{
    static_assert(offsetof(DlHead, slab_stamp) == 184, "ofl_scatter_dev.h: kSlabStampAt");
    int layouts = 0;
    for (const Shape &s : kShapes)
        for (void *base : { (void *)nullptr, reinterpret_cast<void *>((uintptr_t)1 << 40) }) {      // the dry run, and an address (never read)
            if (check(s, base)) return 1;
            ++layouts;
        }
    printf("%d layouts ok\n", layouts);
    return 0;
}
