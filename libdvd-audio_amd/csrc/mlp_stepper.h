// mlp_stepper.h -- streaming tier: the decoder state stays on the device (mlp_step.h; host side: mlp_stream.c).
// One call decodes one packet's access units by one workgroup of the cooperative kernel (mlp_coop.h).
#pragma once
#include <string.h>
#include <new>

#include "hip_ws.h"
#include "mlp_check.h"
#include "mlp_coop.h"
#include "mlp_step.h"

using namespace mlp;

struct StepDesc {           // what the host writes in front of the packet's bytes: a one-segment index made by hand
    SegRec seg;
    StreamRec streams;
    uint32_t seg_fbase[2];
    uint32_t n_seg;
    uint32_t state_valid;   // (informational: whether the decoder had state; the kernel is told by DecodeArgs::coop_fresh)
    uint64_t out_off, out_stride;
    uint32_t cls[4];
};
constexpr size_t STEP_DESC_BYTES = 256;
static_assert(sizeof(StepDesc) <= STEP_DESC_BYTES, "the descriptor fits its place");
static_assert(sizeof(dvda_mlp_step_result) == sizeof(CoopResult), "the result record is the kernel's");
constexpr size_t STEP_PCM_BYTES = (size_t)DVDA_STEP_MAX_UNITS * 160u * 6u * 4u;

struct dvda_mlp_hip_stepper {
    int device = 0;
    Stream st;
    uint8_t *d_in = nullptr;    // [StepDesc | bytes + 64]: the device's view of h_in (pinned host memory: the kernels read the
                                // packet where the host put it -- 2 KB over PCIe costs less than a copy's launch)
    DevBuf<uint8_t> d_masks;
    DevBuf<uint16_t> d_parts;
    DevBuf<uint32_t> d_tile_count;  // [2]
    DevBuf<uint32_t> d_small;       // seg_check[2] | seg_status | seg_rows | yield | seg_meta[2]
    DevBuf<DecodeSummary> d_summary;
    DevBuf<CoopState> d_state;      // [2]
    uint8_t *d_out = nullptr;   // [CoopResult | pcm]: the device's view of h_out (the PCM is written where the host reads it)
    uint8_t *h_in = nullptr, *h_out = nullptr;  // pinned, mapped

    ~dvda_mlp_hip_stepper()
    {
        (void)hipHostFree(h_in);
        (void)hipHostFree(h_out);
    }
};

// parity / CRC-8 of the step's access units by ONE workgroup: the per-chunk partial sums (k_sync_mask's, mlp_index.h),
// then the substreams' checks from them (k_au_check's, mlp_check.h) -- two launches of the batch tier, here one
__global__ __launch_bounds__(IDX_THREADS) void k_step_check(const uint8_t *__restrict__ bytes, uint32_t total_bytes,
                                                            uint16_t *__restrict__ parts, const StepDesc *__restrict__ d,
                                                            uint32_t *__restrict__ seg_check)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_slice[16 * 256];
    __shared__ __attribute__((aligned(16))) uint8_t s_log[256];
    __shared__ __attribute__((aligned(16))) uint8_t s_exp[512];
    for (int i = threadIdx.x; i < 16 * 256 / 16; i += IDX_THREADS)
        reinterpret_cast<uint4 *>(s_slice)[i] = reinterpret_cast<const uint4 *>(d_chk.slice)[i];
    for (int i = threadIdx.x; i < 256 / 16; i += IDX_THREADS)
        reinterpret_cast<uint4 *>(s_log)[i] = reinterpret_cast<const uint4 *>(d_chk.log)[i];
    for (int i = threadIdx.x; i < 512 / 16; i += IDX_THREADS)
        reinterpret_cast<uint4 *>(s_exp)[i] = reinterpret_cast<const uint4 *>(d_chk.exp)[i];
    __syncthreads();
    const uint32_t n_chunks = (total_bytes + 15u) >> 4;
    for (uint32_t chunk = threadIdx.x; chunk < n_chunks; chunk += IDX_THREADS) {
        uint32_t part;
        (void)mask_chunk(bytes, total_bytes, chunk, s_slice, part);
        parts[chunk] = (uint16_t)part;
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x < (uint32_t)CHK_GROUP)
        au_check_group(0, threadIdx.x, bytes, parts, &d->seg, &d->streams, seg_check, s_slice, s_log, s_exp);
}

extern "C" void dvda_mlp_hip_stepper_destroy(dvda_mlp_hip_stepper *s)
{
    if (!s)
        return;
    (void)hipSetDevice(s->device);
    if (s->st)
        (void)hipStreamSynchronize(s->st);
    delete s;
}

extern "C" int dvda_mlp_hip_stepper_create(dvda_mlp_hip_stepper **out, int device)
{
    if (!out)
        return DVDA_HIP_EINVAL;
    *out = nullptr;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
        return DVDA_HIP_ENODEV;
    dvda_mlp_hip_stepper *s = new (std::nothrow) dvda_mlp_hip_stepper();
    if (!s)
        return DVDA_HIP_ENOMEM;
    s->device = device;
    const size_t in_bytes = STEP_DESC_BYTES + DVDA_STEP_MAX_BYTES + 128;
    const size_t chunks = (DVDA_STEP_MAX_BYTES + 128) / 16 + 8;
    const size_t out_bytes = sizeof(CoopResult) + STEP_PCM_BYTES;
    bool ok = hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(s->st.put(), hipStreamNonBlocking) == hipSuccess &&
              s->d_masks.alloc(chunks) == hipSuccess && s->d_parts.alloc(chunks) == hipSuccess &&
              s->d_tile_count.alloc(4) == hipSuccess && s->d_small.alloc(16) == hipSuccess &&
              s->d_summary.alloc(1 + SUMMARY_PARTS) == hipSuccess && s->d_state.alloc(2) == hipSuccess &&
              hipHostMalloc((void **)&s->h_in, in_bytes, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
              hipHostMalloc((void **)&s->h_out, out_bytes, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
              hipHostGetDevicePointer((void **)&s->d_in, s->h_in, 0) == hipSuccess &&
              hipHostGetDevicePointer((void **)&s->d_out, s->h_out, 0) == hipSuccess;
    ok = ok && hipMemset(s->d_state, 0, 2 * sizeof(CoopState)) == hipSuccess &&
         hipMemset(s->d_summary, 0, (1 + SUMMARY_PARTS) * sizeof(DecodeSummary)) == hipSuccess &&
         hipMemset(s->d_small, 0, 16 * sizeof(uint32_t)) == hipSuccess;
    if (!ok) {
        dvda_mlp_hip_stepper_destroy(s);
        return DVDA_HIP_ENODEV;         // no GPU (or no memory on it): there is no CPU decoder here
    }
    memset(s->h_in, 0, in_bytes);
    memset(s->h_out, 0, out_bytes);
    *out = s;
    return DVDA_HIP_OK;
}

extern "C" int dvda_mlp_hip_stepper_step(dvda_mlp_hip_stepper *s, const uint8_t *bytes, size_t len, uint32_t n_units,
                                         uint32_t packed_sync, int fresh, const dvda_mlp_step_result **res,
                                         const int32_t **pcm, uint64_t *stride, unsigned *channels)
{
    if (!s || !bytes || !res || !pcm || !stride || len == 0 || n_units == 0)
        return DVDA_HIP_EINVAL;
    if (len > DVDA_STEP_MAX_BYTES || n_units > DVDA_STEP_MAX_UNITS)
        return DVDA_HIP_ECAPACITY;
    const uint32_t rpa = rows_per_au((packed_sync >> 8) & 0xFu);
    const uint32_t nch = channel_count((packed_sync >> 16) & 0x1Fu);
    if (rpa == 0 || nch == 0)
        return DVDA_HIP_EINVAL;
    HIP_TRY(hipSetDevice(s->device));
    const uint64_t rows_cap = (uint64_t)n_units * rpa;
    // ---- the hand-made index of one segment + the bytes, up in one copy
    StepDesc *d = reinterpret_cast<StepDesc *>(s->h_in);
    memset(d, 0, sizeof(*d));
    d->seg.off = 0;
    d->seg.end = len;
    d->seg.stream = 0;
    d->seg.nframes = n_units;
    d->seg.flags = SEG_STREAMING;
    d->seg.sync = packed_sync;
    d->seg.ndrop = 0;
    d->seg.prev = 0xFFFFFFFFu;
    d->streams.first_seg = 0;
    d->streams.n_seg = 1;
    d->streams.sync = packed_sync;
    d->seg_fbase[0] = 0;
    d->seg_fbase[1] = n_units;
    d->n_seg = 1;
    d->state_valid = fresh ? 0u : 1u;
    d->out_off = 0;
    d->out_stride = rows_cap;
    d->cls[0] = d->cls[1] = 1;
    uint8_t *hb = s->h_in + STEP_DESC_BYTES;
    memcpy(hb, bytes, len);
    memset(hb + len, 0, 128);
    const StepDesc *dd = reinterpret_cast<const StepDesc *>(s->d_in);
    const uint8_t *d_bytes = s->d_in + STEP_DESC_BYTES;
    // ---- parity / CRC-8: per-chunk partial sums, joined per substream (mlp_check.h)
    hipLaunchKernelGGL(k_step_check, dim3(1), dim3(IDX_THREADS), 0, s->st, d_bytes, (uint32_t)len, s->d_parts, dd, s->d_small);
    // ---- the units themselves: one workgroup, state in, state out
    DecodeArgs a;
    memset(&a, 0, sizeof(a));
    a.bytes = d_bytes;
    a.total_bytes = len;
    a.seg = &dd->seg;
    a.seg_fbase = dd->seg_fbase;
    a.n_seg_ptr = &dd->n_seg;
    a.max_seg = 1;
    a.streams = const_cast<StreamRec *>(&dd->streams);
    a.pcm = reinterpret_cast<int32_t *>(s->d_out + sizeof(CoopResult));
    a.out_off = &dd->out_off;
    a.out_stride = &dd->out_stride;
    a.seg_status = s->d_small + 2;
    a.seg_rows = s->d_small + 3;
    a.yield_req = s->d_small + 4;
    a.seg_meta = s->d_small + 5;
    a.seg_check = s->d_small;
    a.total_lanes = 2;
    a.summary = s->d_summary;
    a.cls = dd->cls;
    a.coop = 64;
    a.caps.max_seg = 1;
    a.caps.max_streams = 1;
    a.caps.lanes = 2;
    a.coop_state = s->d_state;
    a.coop_result = reinterpret_cast<CoopResult *>(s->d_out);
    a.coop_fresh = fresh ? 1u : 0u;
    hipLaunchKernelGGL((k_coop<false, true>), dim3(1), dim3(COOP_THREADS), 0, s->st, a);
    HIP_TRY(hipStreamSynchronize(s->st));       // (the kernel's stores to host memory are there when it has ended)
    *res = reinterpret_cast<const dvda_mlp_step_result *>(s->h_out);
    *pcm = reinterpret_cast<const int32_t *>(s->h_out + sizeof(CoopResult));
    *stride = rows_cap;
    if (channels)
        *channels = nch;
    return DVDA_HIP_OK;
}
