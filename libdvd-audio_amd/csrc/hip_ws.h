// hip_ws.h -- host side: what the library owns on a device, each thing freed by the destructor of the member that
// holds it.  A context (mlp_ctx.h) lists its workspaces once, as members; nothing is freed by hand.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/dvda_mlp_hip.h"

#define HIP_TRY(x)                                                                         \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) {                                                            \
            fprintf(stderr, "dvda_mlp_hip: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), \
                    __FILE__, __LINE__);                                                   \
            return DVDA_HIP_ENODEV;                                                        \
        }                                                                                  \
    } while (0)

// Debug aid: DVDA_POISON=<byte> fills every workspace this library allocates with that byte, so a kernel that
// reads what no kernel wrote shows itself the same way on every run (tools/soak_reuse.py uses it).
static hipError_t ws_malloc(void **p, size_t bytes)
{
    static const int poison = getenv("DVDA_POISON") ? (int)strtol(getenv("DVDA_POISON"), nullptr, 0) : -1;
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess && poison >= 0)
        e = hipMemset(*p, poison & 0xFF, bytes);
    return e;
}

struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};

// a device buffer and how many elements it holds; reads as a T * wherever one is expected
template <typename T>
struct DevBuf : NoCopy {
    T *p = nullptr;
    uint64_t cap = 0;           // elements

    ~DevBuf() { (void)hipFree(p); }
    operator T *() const { return p; }
    T *operator->() const { return p; }

    void release()
    {
        (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    // exactly n elements, whatever it held
    hipError_t alloc(uint64_t n)
    {
        release();
        const hipError_t e = ws_malloc((void **)&p, n * sizeof(T));
        if (e == hipSuccess)
            cap = n;
        return e;
    }
    // at least `need` elements, exactly that many when it has to be allocated anew (the old content is gone)
    int grow_exact(uint64_t need)
    {
        if (need <= cap)
            return DVDA_HIP_OK;
        return alloc(need) == hipSuccess ? DVDA_HIP_OK : DVDA_HIP_ENOMEM;
    }
    // ... with room to spare: outside the common path (the first batch that needs it), so that batches a little
    // larger than the last do not allocate again
    int grow(uint64_t need) { return need <= cap ? DVDA_HIP_OK : grow_exact(need + need / 8 + 1024); }
};

// a runtime handle destroyed with its owner
template <typename H, hipError_t (*Destroy)(H)>
struct Owned : NoCopy {
    H h = nullptr;

    ~Owned() { reset(); }
    operator H() const { return h; }
    H *put()                    // for the call that creates it (what it held is destroyed first)
    {
        reset();
        return &h;
    }
    void reset()
    {
        if (h)
            (void)Destroy(h);
        h = nullptr;
    }
};
using Event = Owned<hipEvent_t, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using GraphExec = Owned<hipGraphExec_t, hipGraphExecDestroy>;
