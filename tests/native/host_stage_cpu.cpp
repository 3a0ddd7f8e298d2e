// Host build of the staging layout (oflibnumpy_amd/csrc/ofl_stage_layout.h, the very header ofl_host_stage.h includes) over
// the part lists of the eight host-array entry points.  Stand-alone: exits 0 and prints the number of layouts checked, or
// prints the first broken rule and exits 1.  tests/test_host_stage.py builds it with -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "../../oflibnumpy_amd/csrc/ofl_stage_layout.h"

namespace {

enum Kind { IN, OUT, SCRATCH };
enum Unit { PX, BATCH, BYTES };         // what `per` multiplies: pixels of the call, fields of the call, or nothing

struct Spec { const char *name; Kind kind; Unit unit; size_t per; bool optional; };
struct Entry { const char *name; std::vector<Spec> parts; };

// element sizes: masks 1, the fill workspace 2, scalars 4, vectors 8, one error record 96 bytes
const std::vector<Entry> kEntries = {
    { "ofl_compose3", { { "fa", IN, PX, 8, false }, { "fb", IN, PX, 8, false }, { "ma", IN, PX, 1, false }, { "mb", IN, PX, 1, false },
                        { "out", OUT, PX, 8, false }, { "mout", OUT, PX, 1, false }, { "stats", OUT, BATCH, 8, true } } },
    { "ofl_gather_bilinear", { { "src", IN, PX, 4, false }, { "flow", IN, PX, 8, false }, { "smask", IN, PX, 1, true }, { "fmask", IN, PX, 1, true },
                               { "dst", OUT, PX, 4, false }, { "valid", OUT, PX, 1, true } } },
    { "ofl_scatter_linear", { { "flow", IN, PX, 8, false }, { "vals", IN, PX, 4, true }, { "query", IN, PX, 8, true }, { "pmask", IN, PX, 1, true },
                              { "vmask", IN, PX, 1, true }, { "out", OUT, PX, 4, true }, { "valid", OUT, PX, 1, true },
                              { "workspace", SCRATCH, BYTES, 4096 + 512, false } } },
    { "ofl_flow_stats", { { "flow", IN, PX, 8, false }, { "mask", IN, PX, 1, true }, { "stats", OUT, BYTES, 4, false } } },
    { "ofl_resize_flow", { { "vecs", IN, PX, 8, false }, { "mask", IN, PX, 1, true }, { "out", OUT, PX, 8, false }, { "mout", OUT, PX, 1, true } } },
    { "ofl_consistency", { { "f", IN, PX, 8, false }, { "b", IN, PX, 8, false }, { "fm", IN, PX, 1, false }, { "bm", IN, PX, 1, false },
                           { "consistent", OUT, PX, 1, false }, { "covered", OUT, PX, 1, true }, { "residual", OUT, PX, 4, true },
                           { "counts", OUT, BATCH, 8, true } } },
    { "ofl_flow_error", { { "est", IN, PX, 8, false }, { "gt", IN, PX, 8, false }, { "est_mask", IN, PX, 1, true }, { "gt_mask", IN, PX, 1, false },
                          { "workspace", SCRATCH, BATCH, 96, false }, { "records", OUT, BATCH, 96, false }, { "epe_map", OUT, PX, 4, true },
                          { "outlier_map", OUT, PX, 1, true } } },
    { "ofl_fill", { { "vecs", IN, PX, 8, true }, { "mask", IN, PX, 1, false }, { "valid", IN, PX, 1, true }, { "workspace", SCRATCH, PX, 2, false },
                    { "out_vecs", OUT, PX, 8, true }, { "out_mask", OUT, PX, 1, true }, { "index", OUT, PX, 4, true }, { "d2", OUT, PX, 4, true } } },
};

int broken(const char *entry, size_t n, unsigned absent, const char *rule, const char *a, const char *b = "")
{
    printf("%s, %zu px, absent set 0x%x: %s (%s %s)\n", entry, n, absent, rule, a, b);
    return 1;
}

// one layout: the optional parts whose bit in `absent` is set are left out; n == 0 makes every part a zero-byte one
int check(const Entry &e, size_t n, size_t batch, unsigned absent)
{
    static char host[1];                 // any non-null host address: the layout never reads through it
    ofl::StageLayout lay;
    std::vector<int> idx;
    std::vector<bool> want;
    unsigned bit = 0;
    for (const Spec &s : e.parts) {
        const bool present = !(s.optional && ((absent >> bit) & 1u));
        if (s.optional) ++bit;
        const size_t bytes = n == 0 ? 0 : s.per * (s.unit == PX ? n : s.unit == BATCH ? batch : 1);
        want.push_back(present);
        idx.push_back(s.kind == IN ? lay.input(present ? host : nullptr, bytes)
                    : s.kind == OUT ? lay.output(present ? host : nullptr, bytes)
                                    : lay.scratch(bytes, present));
    }
    if (lay.total() == 0) return broken(e.name, n, absent, "the total is 0", "");
    size_t used = 0;
    for (size_t i = 0; i < idx.size(); ++i) {
        const ofl::StagePart &p = lay.parts[idx[i]];
        if (p.present != want[i]) return broken(e.name, n, absent, "presence differs from what was declared", e.parts[i].name);
        if (!p.present) continue;
        if (p.offset % 16) return broken(e.name, n, absent, "offset off the 16-byte grid", e.parts[i].name);
        if (p.offset + p.bytes + 16 > lay.total()) return broken(e.name, n, absent, "slack runs past the allocation", e.parts[i].name);
        used += p.bytes + 16;
        for (size_t j = 0; j < i; ++j) {
            const ofl::StagePart &q = lay.parts[idx[j]];
            if (!q.present) continue;
            // [offset, offset + bytes + 16) of any two present parts are disjoint: no overlap, 16 bytes of slack each,
            // and distinct addresses for zero-byte parts
            if (p.offset < q.offset + q.bytes + 16 && q.offset < p.offset + p.bytes + 16)
                return broken(e.name, n, absent, "two parts overlap or share their slack", e.parts[i].name, e.parts[j].name);
        }
    }
    // absent parts take no space: what is allocated is the present parts, their slack and less than 16 bytes of padding each
    size_t n_present = 0;
    for (size_t i = 0; i < idx.size(); ++i) n_present += want[i] ? 1 : 0;
    if (n_present && lay.total() >= used + 16 * n_present) return broken(e.name, n, absent, "more space than the present parts need", "");
    return 0;
}

}  // namespace

int main()
{
    const size_t pixels[] = { 0, 1, 15, 16, 17, 1 + 2 * 3 * 5 * 7 };       // 0: zero-byte present parts
    long layouts = 0;
    for (const Entry &e : kEntries) {
        unsigned n_opt = 0;
        for (const Spec &s : e.parts) n_opt += s.optional ? 1 : 0;
        for (size_t n : pixels)
            for (size_t batch : { (size_t)1, (size_t)3 })
                for (unsigned absent = 0; absent < (1u << n_opt); ++absent, ++layouts)
                    if (check(e, n * batch, batch, absent)) return 1;
    }
    ofl::StageLayout none;
    if (none.total() == 0) { printf("an empty layout has total 0\n"); return 1; }
    printf("%ld layouts ok\n", layouts);
    return 0;
}
