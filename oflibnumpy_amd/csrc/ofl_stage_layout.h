// ofl_stage_layout.h -- where the parts of one host-array call lie in its single device allocation.  Pure host
// arithmetic, nothing of HIP: tests/native/host_stage_cpu.cpp compiles it with plain g++.
#pragma once
#include <stddef.h>
#include <vector>

namespace ofl {

// Every present part starts on this boundary and is followed by at least as many bytes that belong to no other part (the
// kernels' paired loads may read past a part's end).  The _dev entries pick their kernel by the alignment of the pointers
// they are given, so this constant decides the route of every host-array call: with 16, `px2` in ofl_consistency_dev is
// W % 2 == 0, `wide` in ofl_flow_error_dev is batch == 1 || H * W % 4 == 0, and the alignment refusals of ofl_fill_dev,
// ofl_flow_error_dev and ofl_consistency_dev cannot fire.  Whoever lowers it changes those routes.
constexpr size_t kStageAlign = 16;

struct StagePart {
    const void *src;      // input: the host source
    void       *dst;      // output: the host destination
    size_t      bytes, offset;
    bool        present;  // an absent part (NULL host pointer, scratch not asked for) takes no space
    bool        zero;     // cleared on the device before the launch
};

struct StageLayout {
    std::vector<StagePart> parts;
    size_t end = 0;

    int input(const void *src, size_t bytes)                  { return add({ src, nullptr, bytes, 0, src != nullptr, false }); }
    int output(void *dst, size_t bytes, bool zero = false)    { return add({ nullptr, dst, bytes, 0, dst != nullptr, zero }); }
    int scratch(size_t bytes, bool wanted = true, bool zero = false) { return add({ nullptr, nullptr, bytes, 0, wanted, zero }); }

    size_t total() const { return end ? end : kStageAlign; }      // never 0

private:
    int add(StagePart p)
    {
        if (p.present) {
            p.offset = end;
            end = (end + p.bytes + 2 * kStageAlign - 1) / kStageAlign * kStageAlign;      // a part of zero bytes still owns its address
        }
        parts.push_back(p);
        return (int)parts.size() - 1;
    }
};

}  // namespace ofl
