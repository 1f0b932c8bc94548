// Host-side helpers every operator's entry points share: the refusal of a bad argument and the layout of a caller-provided workspace.
#pragma once
#include "common.h"

#include <stddef.h>

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Sets the last-error string (with the caller's file and line) and hands the status code back: `return refuse(ROITR_ERR_ARG, "...")`.
static inline int refuse(int code, const char* msg, const char* file = __builtin_FILE(), int line = __builtin_LINE())
{
    roitr_set_error(msg, file, line);
    return code;
}

// Walks a workspace in 256-byte steps.  Every operator has ONE carve function that takes its buffers from a Carve in order; its
// *_workspace_bytes() runs that function against a null base and reads `bytes`, the launcher runs it against the caller's pointer:
// the size cannot miss a buffer the carve takes (the rule engine.cpp states for its arenas).  Against a null base take() returns null.
struct Carve {
    char* base;
    size_t bytes = 0;
    explicit Carve(void* ws) : base(static_cast<char*>(ws)) {}
    template <typename T>
    T* take(size_t count)
    {
        T* q = base ? reinterpret_cast<T*>(base + bytes) : nullptr;
        bytes += align256(count * sizeof(T));
        return q;
    }
    // the caller's pointer rounded up to 256 bytes, for the operators whose size includes 256 bytes of room for that
    static void* aligned(void* ws) { return reinterpret_cast<void*>(align256(reinterpret_cast<size_t>(ws))); }
};
