// Bump allocator over one block of scratch: the only way a pass cuts its buffers out of a workspace.  Host code only.
//
// A layout is a function that takes its buffers from an Arena&, in a fixed order, with the element counts written once.  It runs
// twice over the same sizes: on a measuring arena (null base, unbounded: only `off` moves, the pointers it hands out are null and
// unused) to learn how many bytes to ask for, and on the bound arena over the block that was then allocated (bind_ws, common.h).
// The same sequence of takes gives the same offsets in both runs, so the request and the carve cannot drift apart, and a take
// that does not fit raises `over` instead of handing out an address outside the block.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace yoho {

struct Arena {
    char* base = nullptr;        // null: measuring
    size_t off = 0;              // bytes taken so far (the end of the last buffer)
    size_t cap = SIZE_MAX;       // bytes of the block
    bool over = false;           // sticky: a take did not fit (or its size overflowed size_t)

    // `count` elements of T at the next multiple of `align` (a power of two).  Null when measuring, and when the buffer would end
    // behind `cap`: `over` is raised then, and `off` still advances where it can, so that it tells how much the layout wanted.
    template <typename T>
    T* take(size_t count, size_t align = 256) {
        const size_t start = (off + (align - 1)) & ~(align - 1);
        if (start < off || count > (SIZE_MAX - start) / sizeof(T)) { over = true; return nullptr; }
        off = start + count * sizeof(T);
        if (off > cap) { over = true; return nullptr; }
        return base ? reinterpret_cast<T*>(base + start) : nullptr;
    }
};

}  // namespace yoho
