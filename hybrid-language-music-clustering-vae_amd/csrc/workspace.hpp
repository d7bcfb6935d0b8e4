// Carving one caller-provided workspace into sub-buffers.  An op's layout() walks a Carver once and returns the named
// offsets plus the total; its *_workspace query and the op itself both call that layout(), so the size the caller
// allocates and the offsets the kernels get cannot drift apart.
#pragma once
#include <cstddef>

namespace hlmc {

inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

struct Carver {
    size_t off = 0;   // where the next sub-buffer starts = the bytes taken so far
    // a sub-buffer of exactly `bytes`, the next one directly behind it
    size_t pack(size_t bytes) { return (off += bytes) - bytes; }
    // a sub-buffer whose size is rounded up to 256 bytes (the next one starts aligned if this one did)
    size_t take(size_t bytes) { return pack(align256(bytes)); }
};

}  // namespace hlmc
