// pcm_levels_run.h -- host side of the level report (pcm_levels.h): the launch sequence, the call that runs it behind a
// decode on the context's own workspace, and the host arithmetic that joins two reports.
#pragma once
#include <vector>

#include "mlp_ctx.h"
#include "pcm_levels.h"

// tiles the flat list can hold for n streams of max_total_frames in all: every stream has at most one ragged tile
static inline uint64_t lvl_max_tiles(uint32_t n, uint64_t max_total_frames)
{
    return max_total_frames / lvl::TILE + n;
}

// workspace (uint32 words): tiles per stream [n + 1] | their exclusive scan [n + 1] | block sums of the scan | tile records
extern "C" size_t dvda_pcm_hip_levels_workspace_words(uint32_t n, uint64_t max_total_frames)
{
    return 2 * ((size_t)n + 1) + ((size_t)n + 1023) / 1024 + 2 + (size_t)lvl_max_tiles(n, max_total_frames) * lvl::REC;
}

extern "C" int dvda_pcm_hip_levels(const int32_t *d_pcm, uint32_t layout, unsigned bits, const dvda_pcm_crc_desc *d_desc,
                                   uint32_t n, uint64_t max_total_frames, dvda_pcm_levels *d_levels, uint32_t *d_work,
                                   size_t work_words, void *stream_)
{
    if ((bits != 16 && bits != 20 && bits != 24) || (layout != DVDA_PCM_PLANAR && layout != DVDA_PCM_INTERLEAVED) ||
        !d_pcm || !d_desc || !d_levels || !d_work)
        return DVDA_HIP_EINVAL;
    if (work_words < dvda_pcm_hip_levels_workspace_words(n, max_total_frames))
        return DVDA_HIP_EINVAL;
    const uint64_t max_tiles = lvl_max_tiles(n, max_total_frames);
    if (max_tiles >> 31)
        return DVDA_HIP_ECAPACITY;
    // (asked of the runtime once per process; the arguments are judged first, on any machine)
    static const bool have_device = [] {
        int ndev = 0;
        return hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
    }();
    if (!have_device)
        return DVDA_HIP_ENODEV;
    if (n == 0)
        return DVDA_HIP_OK;
    hipStream_t st = (hipStream_t)stream_;
    uint32_t *cnt = d_work;
    uint32_t *base = cnt + n + 1;
    uint32_t *tmp = base + n + 1;
    uint32_t *rec = tmp + (n + 1023) / 1024 + 2;
    hipLaunchKernelGGL(lvl::k_lvl_plan, dim3((n + 255) / 256), dim3(256), 0, st, d_desc, n, cnt);
    enqueue_exscan(st, cnt, base, tmp, n, nullptr, n);
    const dim3 grid((unsigned)(max_tiles < lvl::TILE_BLOCKS ? max_tiles : lvl::TILE_BLOCKS)), block(lvl::THREADS);
    if (layout == DVDA_PCM_PLANAR)
        hipLaunchKernelGGL(lvl::k_lvl_tiles<true>, grid, block, 0, st, d_pcm, d_desc, n, (uint32_t)bits, base, rec,
                           (uint32_t)max_tiles);
    else
        hipLaunchKernelGGL(lvl::k_lvl_tiles<false>, grid, block, 0, st, d_pcm, d_desc, n, (uint32_t)bits, base, rec,
                           (uint32_t)max_tiles);
    hipLaunchKernelGGL(lvl::k_lvl_join, dim3(n), block, 0, st, d_desc, n, base, rec, (uint32_t)max_tiles, d_levels);
    HIP_TRY(hipGetLastError());
    return DVDA_HIP_OK;
}

extern "C" int dvda_mlp_hip_pcm_levels(dvda_mlp_hip_ctx *c, const int32_t *d_pcm, const uint64_t *d_out_off,
                                       const uint64_t *d_out_stride, unsigned bits, dvda_pcm_levels *host_levels, uint32_t n,
                                       void *stream_)
{
    if (!c || !d_pcm || !d_out_off || !d_out_stride || !host_levels || (bits != 16 && bits != 20 && bits != 24) ||
        (c->set.pcm_layout != DVDA_PCM_PLANAR && c->set.pcm_layout != DVDA_PCM_INTERLEAVED))
        return DVDA_HIP_EINVAL;
    if (!c->indexed)
        return DVDA_HIP_ESTATE;
    if (n > c->n_streams)
        n = c->n_streams;
    if (n == 0)
        return DVDA_HIP_OK;
    hipStream_t st = (hipStream_t)stream_;
    // frames and channels as the caller is told them: conceal mode's composed record and the presentation included
    std::vector<dvda_mlp_stream_info> infos(n);
    int rc = dvda_mlp_hip_stream_info(c, infos.data(), n, stream_);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<uint64_t> off(n), stride(n);
    HIP_TRY(hipMemcpy(off.data(), d_out_off, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(stride.data(), d_out_stride, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    std::vector<dvda_pcm_crc_desc> desc(n);
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) {
        dvda_pcm_crc_desc &d = desc[i];
        d.off = off[i];
        d.stride = stride[i];
        // (an overflowed stream's region does not hold the stream)
        d.frames = (infos[i].status & DVDA_ST_OVERFLOW) ? 0 : infos[i].pcm_frames;
        d.channels = infos[i].channels;
        d.reserved = 0;
        total += d.frames;
    }
    const size_t words = dvda_pcm_hip_levels_workspace_words(n, total);
    if ((rc = c->d_lvl_desc.grow(n)) != 0 || (rc = c->d_lvl_out.grow(n)) != 0 || (rc = c->d_lvl_work.grow(words)) != 0)
        return rc;
    HIP_TRY(hipMemcpy(c->d_lvl_desc, desc.data(), (size_t)n * sizeof(dvda_pcm_crc_desc), hipMemcpyHostToDevice));
    rc = dvda_pcm_hip_levels(d_pcm, c->set.pcm_layout, bits, c->d_lvl_desc, n, total, c->d_lvl_out, c->d_lvl_work,
                             (size_t)c->d_lvl_work.cap, stream_);
    if (rc)
        return rc;
    HIP_TRY(hipMemcpyAsync(host_levels, c->d_lvl_out, (size_t)n * sizeof(dvda_pcm_levels), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DVDA_HIP_OK;
}

extern "C" void dvda_pcm_hip_levels_combine(const dvda_pcm_levels *a_, const dvda_pcm_levels *b_, dvda_pcm_levels *out)
{
    const dvda_pcm_levels a = *a_, b = *b_;         // (either may be `out`)
    if (a.frames == 0 || b.frames == 0) {           // neutral: its zero min / max must not reach the result
        *out = a.frames ? a : b;
        return;
    }
    dvda_pcm_levels r;
    r.frames = a.frames + b.frames;
    r.lead_silent = a.lead_silent == a.frames ? a.frames + b.lead_silent : a.lead_silent;
    r.trail_silent = b.trail_silent == b.frames ? b.frames + a.trail_silent : b.trail_silent;
    for (int c = 0; c < 8; c++) {
        r.sum[c] = (int64_t)((uint64_t)a.sum[c] + (uint64_t)b.sum[c]);
        r.over[c] = a.over[c] + b.over[c];
        r.min[c] = a.min[c] < b.min[c] ? a.min[c] : b.min[c];
        r.max[c] = a.max[c] > b.max[c] ? a.max[c] : b.max[c];
    }
    *out = r;
}
