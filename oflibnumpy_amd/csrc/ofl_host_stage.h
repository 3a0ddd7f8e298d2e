// ofl_host_stage.h -- the one upload / launch / download / clean-up path of the entry points that take host arrays.
//
//     HostStage st("ofl_x");
//     auto da = st.in(a, n);                             // declare the parts; a NULL host pointer = an absent part
//     auto db = st.out(b, n);
//     OFL_TRY(st.upload());                              // one allocation, the inputs copied, the zeroed parts cleared
//     OFL_TRY(ofl_x_dev(da, db, ..., st.stream()));      // parts convert to typed device pointers (NULL where absent)
//     return st.download();                              // the outputs copied back, the stream synchronised
//
// The destructor synchronises the stream and frees, so any early return is safe; it records no error, so the code and the
// ofl_last_error text of a failing _dev entry reach the caller untouched.
#pragma once
#include "ofl_common.h"
#include "ofl_stage_layout.h"
#include <type_traits>

namespace ofl {

// void pointers (images of a run-time element type) are counted in bytes
template <typename T> constexpr size_t stage_elem_bytes() { if constexpr (std::is_void_v<T>) return 1; else return sizeof(T); }

struct HostStage {
    template <typename T> struct Part {
        const HostStage *st; int k;
        operator T *() const { return static_cast<T *>(st->ptr(k)); }
    };

    explicit HostStage(const char *who) : who_(who) {}
    HostStage(const HostStage &) = delete;
    HostStage &operator=(const HostStage &) = delete;
    ~HostStage()
    {
        if (!base_) return;
        (void)hipStreamSynchronize(stream());       // copies of a failed call may still be queued
        (void)hipFree(base_);
    }

    hipStream_t stream() const { return rt().stream; }

    // `count` elements of T (bytes for void pointers)
    template <typename T> Part<const T> in(const T *host, size_t count)  { return { this, lay_.input(host, count * stage_elem_bytes<T>()) }; }
    template <typename T> Part<T> out(T *host, size_t count, bool zero = false) { return { this, lay_.output(host, count * stage_elem_bytes<T>(), zero) }; }
    template <typename T> Part<T> scratch(size_t count, bool wanted = true, bool zero = false) { return { this, lay_.scratch(count * stage_elem_bytes<T>(), wanted, zero) }; }

    int upload()
    {
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&base_), lay_.total());
        if (e != hipSuccess) { base_ = nullptr; return hip_fail(e, who_); }
        for (const StagePart &p : lay_.parts)
            if (p.present && p.src && p.bytes && (e = hipMemcpyAsync(base_ + p.offset, p.src, p.bytes, hipMemcpyHostToDevice, stream())) != hipSuccess)
                return hip_fail(e, who_);
        for (const StagePart &p : lay_.parts)
            if (p.present && p.zero && p.bytes && (e = hipMemsetAsync(base_ + p.offset, 0, p.bytes, stream())) != hipSuccess)
                return hip_fail(e, who_);
        return OFL_OK;
    }

    int download()
    {
        hipError_t e;
        for (const StagePart &p : lay_.parts)
            if (p.present && p.dst && p.bytes && (e = hipMemcpyAsync(p.dst, base_ + p.offset, p.bytes, hipMemcpyDeviceToHost, stream())) != hipSuccess)
                return hip_fail(e, who_);
        if ((e = hipStreamSynchronize(stream())) != hipSuccess) return hip_fail(e, who_);
        return OFL_OK;
    }

private:
    void *ptr(int k) const { const StagePart &p = lay_.parts[k]; return base_ && p.present ? base_ + p.offset : nullptr; }

    const char *who_;
    StageLayout lay_;
    char       *base_ = nullptr;
};

}  // namespace ofl
