// mlp_stepper.h -- streaming tier: the decoder state stays on the device (mlp_step.h; host side: mlp_stream.c).
// One step decodes one packet's access units of every member of a group of decoders, a workgroup of the cooperative
// kernel (mlp_coop.h) per member; a lone decoder is a group of one.
#pragma once
#include <string.h>
#include <new>

#include "hip_ws.h"
#include "mlp_check.h"
#include "mlp_coop.h"
#include "mlp_step.h"

using namespace mlp;

// What the host writes in front of the members' bytes: a hand-made index of n one-segment streams, as the arrays the
// kernels take (member i: segment i of stream i).  One block of mapped pinned memory:
//   [SegRec[n] | StreamRec[n] | out_off[n] | out_stride[n] | seg_fbase[n + 1] | n_seg | cls[4]] (rounded up to 128 bytes)
//   [member 0's slot: bytes, >= 128 zero bytes | member 1's slot | ...]             DVDA_STEP_SLOT_IN_BYTES each
struct StepLayout {
    size_t seg, streams, out_off, out_stride, seg_fbase, n_seg, cls, bytes, total;
    explicit StepLayout(size_t n)
    {
        seg = 0;
        streams = seg + n * sizeof(SegRec);
        out_off = streams + n * sizeof(StreamRec);
        out_stride = out_off + n * sizeof(uint64_t);
        seg_fbase = out_stride + n * sizeof(uint64_t);
        n_seg = seg_fbase + (n + 1) * sizeof(uint32_t);
        cls = n_seg + sizeof(uint32_t);
        bytes = (cls + 4 * sizeof(uint32_t) + 127) & ~(size_t)127;
        total = bytes + n * (size_t)DVDA_STEP_SLOT_IN_BYTES;
    }
};
static_assert(sizeof(SegRec) % 8 == 0 && sizeof(StreamRec) % 8 == 0, "the 64-bit arrays behind them stay aligned");
static_assert(sizeof(dvda_mlp_step_result) == sizeof(CoopResult), "the result record is the kernel's");
static_assert(DVDA_STEP_SLOT_IN_BYTES % 128 == 0, "a slot starts at a 128-byte boundary (au_check_group's blocks)");
// the way out: [CoopResult[n], in the first n * STEP_RES_BYTES bytes | member 0's PCM | member 1's PCM | ...]
constexpr size_t STEP_RES_BYTES = 512;
constexpr size_t STEP_PCM_WORDS = (size_t)DVDA_STEP_MAX_UNITS * 160u * 6u;
static_assert(sizeof(CoopResult) <= STEP_RES_BYTES && STEP_RES_BYTES + STEP_PCM_WORDS * 4 == DVDA_STEP_SLOT_OUT_BYTES, "the slot's two parts");

struct dvda_mlp_hip_stepper {
    int device = 0;
    uint32_t n = 0;             // members
    Stream st;
    uint8_t *d_in = nullptr;    // the device's view of h_in (pinned host memory: the kernels read the packets where the
                                // host put them -- 2 KB over PCIe costs less than a copy's launch)
    DevBuf<uint16_t> d_parts;       // the partial sums of every slot's 16-byte chunks (member i: from chunk i * slot / 16)
    DevBuf<uint32_t> d_small;       // seg_check[2n] | seg_status[n] | seg_rows[n] | yield[n] | seg_meta[2n]
    DevBuf<DecodeSummary> d_summary;
    DevBuf<CoopState> d_state;      // [2n]: member i's substreams at 2i, 2i + 1
    uint8_t *d_out = nullptr;   // the device's view of h_out (results and PCM are written where the host reads them)
    uint8_t *h_in = nullptr, *h_out = nullptr;  // pinned, mapped

    ~dvda_mlp_hip_stepper()
    {
        (void)hipHostFree(h_in);
        (void)hipHostFree(h_out);
    }
};

// parity / CRC-8 of the step's access units, workgroup i for member i: the per-chunk partial sums of its slot
// (k_sync_mask's, mlp_index.h), then the substreams' checks from them (k_au_check's, mlp_check.h) -- two launches of the
// batch tier, here one.  A member that sits this step out (nframes == 0) costs its workgroup one load.
__global__ __launch_bounds__(IDX_THREADS) void k_step_check(const uint8_t *__restrict__ bytes, uint16_t *__restrict__ parts,
                                                            const SegRec *__restrict__ seg,
                                                            const StreamRec *__restrict__ streams,
                                                            uint32_t *__restrict__ seg_check)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_slice[16 * 256];
    __shared__ __attribute__((aligned(16))) uint8_t s_log[256];
    __shared__ __attribute__((aligned(16))) uint8_t s_exp[512];
    const uint32_t m = blockIdx.x;
    const uint64_t off = seg[m].off, end = seg[m].end;      // (off: the slot's start, a multiple of 128)
    if (seg[m].nframes == 0)
        return;                                             // (the whole workgroup: no barrier is left behind)
    for (int i = threadIdx.x; i < 16 * 256 / 16; i += IDX_THREADS)
        reinterpret_cast<uint4 *>(s_slice)[i] = reinterpret_cast<const uint4 *>(d_chk.slice)[i];
    for (int i = threadIdx.x; i < 256 / 16; i += IDX_THREADS)
        reinterpret_cast<uint4 *>(s_log)[i] = reinterpret_cast<const uint4 *>(d_chk.log)[i];
    for (int i = threadIdx.x; i < 512 / 16; i += IDX_THREADS)
        reinterpret_cast<uint4 *>(s_exp)[i] = reinterpret_cast<const uint4 *>(d_chk.exp)[i];
    __syncthreads();
    const uint32_t chunk0 = (uint32_t)(off >> 4), chunk1 = (uint32_t)((end + 15u) >> 4);
    for (uint32_t chunk = chunk0 + threadIdx.x; chunk < chunk1; chunk += IDX_THREADS) {
        uint32_t part;
        (void)mask_chunk(bytes, end, chunk, s_slice, part);
        parts[chunk] = (uint16_t)part;
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x < (uint32_t)CHK_GROUP)
        au_check_group(m, threadIdx.x, bytes, parts, seg, streams, seg_check, s_slice, s_log, s_exp);
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

extern "C" int dvda_mlp_hip_stepper_create(dvda_mlp_hip_stepper **out, unsigned n, int device)
{
    if (!out)
        return DVDA_HIP_EINVAL;
    *out = nullptr;
    if (n == 0 || n > DVDA_STEP_MAX_MEMBERS)
        return DVDA_HIP_EINVAL;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
        return DVDA_HIP_ENODEV;
    dvda_mlp_hip_stepper *s = new (std::nothrow) dvda_mlp_hip_stepper();
    if (!s)
        return DVDA_HIP_ENOMEM;
    s->device = device;
    s->n = n;
    const StepLayout L(n);
    // (au_check_group reads its partial sums 16 bytes at a time, a run of chunks past a unit's last: 64 chunks of margin)
    const size_t chunks = (size_t)n * DVDA_STEP_SLOT_IN_BYTES / 16 + 64;
    const size_t out_bytes = (size_t)n * DVDA_STEP_SLOT_OUT_BYTES;
    bool ok = hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(s->st.put(), hipStreamNonBlocking) == hipSuccess &&
              s->d_parts.alloc(chunks) == hipSuccess && s->d_small.alloc(7 * (size_t)n) == hipSuccess &&
              s->d_summary.alloc(1 + SUMMARY_PARTS) == hipSuccess && s->d_state.alloc(2 * (size_t)n) == hipSuccess &&
              hipHostMalloc((void **)&s->h_in, L.total, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
              hipHostMalloc((void **)&s->h_out, out_bytes, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
              hipHostGetDevicePointer((void **)&s->d_in, s->h_in, 0) == hipSuccess &&
              hipHostGetDevicePointer((void **)&s->d_out, s->h_out, 0) == hipSuccess;
    ok = ok && hipMemset(s->d_state, 0, 2 * (size_t)n * sizeof(CoopState)) == hipSuccess &&
         hipMemset(s->d_parts, 0, chunks * sizeof(uint16_t)) == hipSuccess &&
         hipMemset(s->d_summary, 0, (1 + SUMMARY_PARTS) * sizeof(DecodeSummary)) == hipSuccess &&
         hipMemset(s->d_small, 0, 7 * (size_t)n * sizeof(uint32_t)) == hipSuccess;
    if (!ok) {
        dvda_mlp_hip_stepper_destroy(s);
        return DVDA_HIP_ENODEV;         // no GPU (or no memory on it): there is no CPU decoder here
    }
    memset(s->h_in, 0, L.total);
    memset(s->h_out, 0, out_bytes);
    // ---- what never changes of the hand-made index: member i is segment i, the only one of stream i; its bytes begin
    //      at its slot, its PCM at its slot; no member has units yet
    SegRec *seg = reinterpret_cast<SegRec *>(s->h_in + L.seg);
    StreamRec *streams = reinterpret_cast<StreamRec *>(s->h_in + L.streams);
    uint64_t *out_off = reinterpret_cast<uint64_t *>(s->h_in + L.out_off);
    uint32_t *cls = reinterpret_cast<uint32_t *>(s->h_in + L.cls);
    for (uint32_t i = 0; i < n; i++) {
        seg[i].off = seg[i].end = (uint64_t)i * DVDA_STEP_SLOT_IN_BYTES;
        seg[i].stream = i;
        seg[i].prev = 0xFFFFFFFFu;
        streams[i].first_seg = i;
        streams[i].n_seg = 1;
        out_off[i] = ((size_t)n * STEP_RES_BYTES + (size_t)i * STEP_PCM_WORDS * 4) / 4;     // (in PCM words from a.pcm = d_out)
    }
    cls[0] = cls[1] = 1;
    *out = s;
    return DVDA_HIP_OK;
}

// One step of the group: the ONE launch sequence of the streaming tier (a lone decoder is the group of one member)
extern "C" int dvda_mlp_hip_stepper_step(dvda_mlp_hip_stepper *s, dvda_mlp_step_item *items, unsigned n_items)
{
    if (!s || (n_items && !items))
        return DVDA_HIP_EINVAL;
    const StepLayout L(s->n);
    SegRec *seg = reinterpret_cast<SegRec *>(s->h_in + L.seg);
    StreamRec *streams = reinterpret_cast<StreamRec *>(s->h_in + L.streams);
    uint64_t *out_stride = reinterpret_cast<uint64_t *>(s->h_in + L.out_stride);
    // ---- the hand-made index: every member sits out (no units) but those of the items this step takes
    for (uint32_t i = 0; i < s->n; i++)
        seg[i].nframes = 0;
    uint32_t n_seg = 0;                 // 1 + the last member that takes part: the grid
    for (unsigned k = 0; k < n_items; k++) {
        dvda_mlp_step_item &it = items[k];
        it.res = nullptr;
        it.pcm = nullptr;
        it.stride = 0;
        it.channels = 0;
        const uint32_t rpa = rows_per_au((it.packed_sync >> 8) & 0xFu);
        const uint32_t nch = channel_count((it.packed_sync >> 16) & 0x1Fu);
        if (it.member >= s->n || !it.bytes || it.len == 0 || it.n_units == 0 || rpa == 0 || nch == 0 ||
            seg[it.member].nframes != 0)
            it.rc = DVDA_HIP_EINVAL;
        else if (it.len > DVDA_STEP_MAX_BYTES || it.n_units > DVDA_STEP_MAX_UNITS)
            it.rc = DVDA_HIP_ECAPACITY;
        else
            it.rc = DVDA_HIP_OK;
        if (it.rc != DVDA_HIP_OK)
            continue;
        const uint32_t m = it.member;
        SegRec &r = seg[m];
        r.end = r.off + it.len;
        r.nframes = it.n_units;
        r.flags = SEG_STREAMING | (it.fresh ? SEG_FRESH : 0u);
        r.sync = it.packed_sync;
        streams[m].sync = it.packed_sync;
        out_stride[m] = (uint64_t)it.n_units * rpa;
        uint8_t *hb = s->h_in + L.bytes + (size_t)m * DVDA_STEP_SLOT_IN_BYTES;
        memcpy(hb, it.bytes, it.len);
        memset(hb + it.len, 0, 128);
        it.stride = out_stride[m];
        it.channels = nch;
        if (m + 1 > n_seg)
            n_seg = m + 1;
    }
    if (n_seg == 0)
        return DVDA_HIP_OK;
    *reinterpret_cast<uint32_t *>(s->h_in + L.n_seg) = n_seg;
    HIP_TRY(hipSetDevice(s->device));
    const uint8_t *d_bytes = s->d_in + L.bytes;         // (segment offsets count from the first slot)
    const SegRec *d_seg = reinterpret_cast<const SegRec *>(s->d_in + L.seg);
    const StreamRec *d_streams = reinterpret_cast<const StreamRec *>(s->d_in + L.streams);
    uint32_t *const small = s->d_small;
    const size_t n = s->n;
    // ---- parity / CRC-8: per-chunk partial sums, joined per substream (mlp_check.h)
    hipLaunchKernelGGL(k_step_check, dim3(n_seg), dim3(IDX_THREADS), 0, s->st, d_bytes, s->d_parts, d_seg, d_streams, small);
    // ---- the units themselves: a workgroup per member, state in, state out
    DecodeArgs a;
    memset(&a, 0, sizeof(a));
    a.bytes = d_bytes;
    a.total_bytes = n * (uint64_t)DVDA_STEP_SLOT_IN_BYTES;
    a.seg = d_seg;
    a.seg_fbase = reinterpret_cast<const uint32_t *>(s->d_in + L.seg_fbase);       // (all zero: a stream's one segment)
    a.n_seg_ptr = reinterpret_cast<const uint32_t *>(s->d_in + L.n_seg);
    a.max_seg = s->n;
    a.streams = const_cast<StreamRec *>(d_streams);
    a.pcm = reinterpret_cast<int32_t *>(s->d_out);
    a.out_off = reinterpret_cast<const uint64_t *>(s->d_in + L.out_off);
    a.out_stride = reinterpret_cast<const uint64_t *>(s->d_in + L.out_stride);
    a.seg_check = small;
    a.seg_status = small + 2 * n;
    a.seg_rows = small + 3 * n;
    a.yield_req = small + 4 * n;
    a.seg_meta = small + 5 * n;
    a.total_lanes = 2 * s->n;
    a.summary = s->d_summary;
    a.cls = reinterpret_cast<const uint32_t *>(s->d_in + L.cls);
    a.coop = 64;
    a.caps.max_seg = s->n;
    a.caps.max_streams = s->n;
    a.caps.lanes = 2 * s->n;
    a.coop_state = s->d_state;
    a.coop_result = reinterpret_cast<CoopResult *>(s->d_out);
    hipLaunchKernelGGL((k_coop<false, true>), dim3(n_seg), dim3(COOP_THREADS), 0, s->st, a);
    HIP_TRY(hipStreamSynchronize(s->st));       // (the kernel's stores to host memory are there when it has ended)
    for (unsigned k = 0; k < n_items; k++) {
        dvda_mlp_step_item &it = items[k];
        if (it.rc != DVDA_HIP_OK)
            continue;
        it.res = reinterpret_cast<const dvda_mlp_step_result *>(s->h_out) + it.member;
        it.pcm = reinterpret_cast<const int32_t *>(s->h_out + n * STEP_RES_BYTES) + (size_t)it.member * STEP_PCM_WORDS;
    }
    return DVDA_HIP_OK;
}
