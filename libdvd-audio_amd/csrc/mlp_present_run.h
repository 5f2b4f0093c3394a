// mlp_present_run.h -- the presentation of substream 0, host side (the kernels: mlp_present.h): the mode switch, the
// strip kernels and the second index behind the source's index, and the getters' view of the inner context's
// findings in the caller's terms.
#pragma once
#include <string.h>

#include "mlp_ctx.h"
#include "mlp_present.h"

extern "C" int dvda_mlp_hip_set_presentation(dvda_mlp_hip_ctx *c, uint32_t presentation)
{
    if (!c || presentation > DVDA_PRESENT_SUBSTREAM0 || (presentation != DVDA_PRESENT_FULL && c->cc.on))
        return DVDA_HIP_EINVAL;
    if (presentation == c->pp.mode)
        return DVDA_HIP_OK;
    if (presentation == DVDA_PRESENT_SUBSTREAM0 && !c->pp.child) {
        HIP_TRY(hipSetDevice(c->device));
        int rc = dvda_mlp_hip_create(&c->pp.child, c->device, c->max_streams, c->max_segments);
        if (rc)
            return rc;
        const size_t ns = c->max_segments, nt = c->max_streams;
        PresentState &p = c->pp;
        hipError_t e = hipSuccess;
        auto alloc = [&](auto &buf, size_t n) {
            if (e == hipSuccess)
                e = buf.alloc(n);
        };
        alloc(p.d_info, nt);
        alloc(p.d_size, ns + 1);
        alloc(p.d_sbase, ns + 1);
        alloc(p.d_len, nt + 1);
        alloc(p.d_base, nt + 1);
        alloc(p.d_off64, nt);
        alloc(p.d_len64, nt);
        for (Event &ev : p.ev)
            if (e == hipSuccess)
                e = hipEventCreate(ev.put());
        if (e != hipSuccess) {
            // (what was allocated stays with the context and is freed with it; the mode stays as it was)
            dvda_mlp_hip_destroy(p.child);
            p.child = nullptr;
            return DVDA_HIP_ENOMEM;
        }
    }
    c->pp.mode = presentation;
    c->indexed = false;             // an index made under the other setting is not this setting's
    c->pp.map_valid = false;
    return DVDA_HIP_OK;
}

// the strip kernels and the second index, enqueued behind the source's index on `st`: no host wait
static int present_index(dvda_mlp_hip_ctx *c, hipStream_t st)
{
    const uint32_t n = c->n_streams, ms = c->max_segments;
    // offsets in the presentation buffer are 32-bit (the scans are)
    const uint64_t bound = ((c->total_bytes + 15) & ~(uint64_t)15) + 16ull * n;
    if (bound + 128 >= (1ull << 32))
        return DVDA_HIP_ECAPACITY;
    c->indexed = false;
    c->pp.map_valid = false;
    if (bound + 128 > c->pp.d_bytes.cap) {
        // (the stream's work so far may still read the old buffer: a second index of an earlier call)
        HIP_TRY(hipStreamSynchronize(st));
        int rc = c->pp.d_bytes.grow(bound + 128);
        if (rc)
            return rc;
    }
    c->pp.bound = bound;
    HIP_TRY(hipEventRecord(c->pp.ev[0], st));
    hipLaunchKernelGGL(k_pp_streams, dim3((n + 255) / 256), dim3(256), 0, st, c->d_bytes, c->d_seg, c->d_streams, n, ms,
                       c->pp.d_info);
    hipLaunchKernelGGL(k_pp_size, dim3((ms + 255) / 256), dim3(256), 0, st, c->d_bytes, c->d_seg, c->d_n_cand, ms,
                       c->pp.d_info, c->pp.d_size);
    enqueue_exscan(st, c->pp.d_size, c->pp.d_sbase, c->d_scan_tmp, 0u, c->d_n_cand, ms);
    hipLaunchKernelGGL(k_pp_len, dim3((n + 255) / 256), dim3(256), 0, st, c->d_streams, n, c->d_n_cand, ms, c->pp.d_info,
                       c->pp.d_sbase, c->pp.d_len, c->pp.d_len64);
    enqueue_exscan(st, c->pp.d_len, c->pp.d_base, c->d_scan_tmp, n, nullptr, n);
    {
        const uint64_t out_bytes = bound + 64, chunks = out_bytes / 16;
        const uint64_t threads = chunks > n ? chunks : n;
        hipLaunchKernelGGL(k_pp_fill, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, c->pp.d_bytes, out_bytes,
                           n, c->pp.d_base, c->pp.d_len64, c->pp.d_off64);
    }
    {
        // one wave per source segment, at most a few waves per SIMD of the device
        uint64_t blocks = ((uint64_t)ms + PP_THREADS / 64 - 1) / (PP_THREADS / 64);
        if (blocks > 4096)
            blocks = 4096;
        hipLaunchKernelGGL(k_pp_copy, dim3((unsigned)blocks), dim3(PP_THREADS), 0, st, c->d_bytes, c->d_seg, c->d_n_cand,
                           ms, c->d_streams, c->pp.d_info, c->pp.d_size, c->pp.d_sbase, c->pp.d_base, c->pp.d_bytes);
    }
    HIP_TRY(hipEventRecord(c->pp.ev[1], st));
    c->pp.ev_set = true;
    HIP_TRY(hipGetLastError());
    const int rc = dvda_mlp_hip_index(c->pp.child, c->pp.d_bytes, bound, c->pp.d_off64, c->pp.d_len64, n, (void *)st);
    if (rc)
        return rc;
    c->indexed = true;
    return DVDA_HIP_OK;
}

extern "C" int dvda_mlp_hip_present_time(dvda_mlp_hip_ctx *c, double *ms, uint64_t *bytes_in, uint64_t *bytes_out)
{
    if (!c || !ms)
        return DVDA_HIP_EINVAL;
    if (!pp_inner(c) || !c->indexed || !c->pp.ev_set)
        return DVDA_HIP_ESTATE;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->pp.ev[1]));
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, c->pp.ev[0], c->pp.ev[1]));
    *ms = t;
    if (bytes_in)
        *bytes_in = c->total_bytes;
    if (bytes_out) {
        uint32_t used = 0;
        HIP_TRY(hipMemcpy(&used, c->pp.d_base + c->n_streams, sizeof(used), hipMemcpyDeviceToHost));
        *bytes_out = used;
    }
    return DVDA_HIP_OK;
}

// diagnostic: the presentation buffer as the second index reads it (the ranges it was given, and the bytes up to what it
// scans plus the 64 behind that); copies only, no state of the context touched
extern "C" int dvda_mlp_hip_present_read(dvda_mlp_hip_ctx *c, uint64_t *offsets, uint64_t *lengths, uint32_t n,
                                         uint64_t *readable, uint8_t *bytes, uint64_t first, uint64_t count, void *stream_)
{
    if (!c)
        return DVDA_HIP_EINVAL;
    if (!pp_inner(c) || !c->indexed)
        return DVDA_HIP_ESTATE;
    const uint64_t limit = c->pp.bound + 64;
    if (first > limit || count > limit - first || (count && !bytes))
        return DVDA_HIP_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream_));
    if (n > c->n_streams)
        n = c->n_streams;
    if (offsets && n)
        HIP_TRY(hipMemcpy(offsets, c->pp.d_off64, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (lengths && n)
        HIP_TRY(hipMemcpy(lengths, c->pp.d_len64, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (readable)
        *readable = limit;
    if (count)
        HIP_TRY(hipMemcpy(bytes, c->pp.d_bytes + first, (size_t)count, hipMemcpyDeviceToHost));
    return DVDA_HIP_OK;
}

// host copies of what the getters map with (once per index call; the caller has waited for `stream`)
static int present_map(dvda_mlp_hip_ctx *c)
{
    if (c->pp.map_valid)
        return DVDA_HIP_OK;
    const uint32_t n = c->n_streams;
    uint32_t nseg = 0;
    HIP_TRY(hipMemcpy(&nseg, c->d_n_cand, sizeof(nseg), hipMemcpyDeviceToHost));
    if (nseg > c->max_segments)
        nseg = c->max_segments;
    c->pp.h_nseg = nseg;
    c->pp.h_seg.resize(nseg);
    c->pp.h_sbase.resize((size_t)nseg + 1);
    c->pp.h_base.resize((size_t)n + 1);
    c->pp.h_info.resize(n);
    c->pp.h_streams.resize(n);
    if (nseg)
        HIP_TRY(hipMemcpy(c->pp.h_seg.data(), c->d_seg, (size_t)nseg * sizeof(SegRec), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(c->pp.h_sbase.data(), c->pp.d_sbase, ((size_t)nseg + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(c->pp.h_base.data(), c->pp.d_base, ((size_t)n + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(c->pp.h_info.data(), c->pp.d_info, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(c->pp.h_streams.data(), c->d_streams, (size_t)n * sizeof(StreamRec), hipMemcpyDeviceToHost));
    c->pp.map_valid = true;
    return DVDA_HIP_OK;
}

static int present_stream_info(dvda_mlp_hip_ctx *c, dvda_mlp_stream_info *infos, uint32_t n, void *stream_)
{
    if (n > c->n_streams)
        n = c->n_streams;
    int rc = dvda_mlp_hip_stream_info(c->pp.child, infos, n, stream_);      // (waits for `stream`)
    if (rc || (rc = present_map(c)) != 0)
        return rc;
    for (uint32_t i = 0; i < n; i++) {
        dvda_mlp_stream_info &o = infos[i];
        const StreamRec &h = c->pp.h_streams[i];
        const uint32_t v = c->pp.h_info[i];
        // what the source says of itself stays the source's
        fill_sync_fields(o, h.sync);
        o.bytes_consumed = h.consumed;
        if (v & (PP_NONE | PP_ENVELOPE)) {
            // no presentation: the source's own finding (or "no k"), nothing decoded
            o.status = h.status | (h.first_seg == 0xFFFFFFFFu ? DVDA_ST_NO_SYNC : 0u) | ((v & PP_ENVELOPE) ? DVDA_ST_ENVELOPE : 0u);
            o.mlp_frames = o.pcm_frames = 0;
            o.segments = 0;
            o.channels = (v & PP_ENVELOPE) ? 0u : channel_count(o.assignment);
        } else {
            o.channels = (v & PP_K_MASK) ? (v & PP_K_MASK) : channel_count(o.assignment);
            o.status |= h.status & (DVDA_ST_TRUNCATED | DVDA_ST_EOF);       // a cut or unframed tail is the source's
        }
    }
    return DVDA_HIP_OK;
}

// a presentation segment's range in the caller's source buffer: its start is the start of the source segment whose
// stripped bytes begin there, its end the end of the source segment its last stripped byte belongs to
static int present_segment_info(dvda_mlp_hip_ctx *c, uint32_t segment, dvda_mlp_segment_info *info, void *stream_)
{
    int rc = dvda_mlp_hip_segment_info(c->pp.child, segment, info, stream_);
    if (rc || (rc = present_map(c)) != 0)
        return rc;
    const uint32_t s = info->stream;
    if (s >= c->n_streams || c->pp.h_streams[s].first_seg >= c->pp.h_nseg)
        return DVDA_HIP_OK;         // (bytes of no stream: the positions stay the presentation buffer's)
    const StreamRec &h = c->pp.h_streams[s];
    const uint32_t lo = h.first_seg, hi = lo + h.n_seg <= c->pp.h_nseg ? lo + h.n_seg : c->pp.h_nseg;
    const uint32_t *sb = c->pp.h_sbase.data();
    if (info->offset < c->pp.h_base[s] || hi <= lo)
        return DVDA_HIP_OK;
    const uint64_t t0 = sb[lo] + (info->offset - c->pp.h_base[s]), t1 = sb[lo] + (info->end - c->pp.h_base[s]);
    // last source segment of the stream that starts at or before t0 (dead ones have no bytes and sort in front of the
    // live one that starts at the same place)
    uint32_t a = lo;
    for (uint32_t l = lo, r = hi; l < r;) {
        const uint32_t m = l + (r - l) / 2;
        if (sb[m] <= t0) {
            a = m;
            l = m + 1;
        } else
            r = m;
    }
    // last one that starts before t1
    uint32_t b = a;
    for (uint32_t l = a, r = hi; l < r;) {
        const uint32_t m = l + (r - l) / 2;
        if (sb[m] < t1) {
            b = m;
            l = m + 1;
        } else
            r = m;
    }
    const bool empty = info->end <= info->offset;
    info->offset = c->pp.h_seg[a].off;
    info->end = empty ? info->offset : c->pp.h_seg[b].end;
    return DVDA_HIP_OK;
}
