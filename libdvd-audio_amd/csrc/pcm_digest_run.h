// pcm_digest_run.h -- host side of the PCM digest (pcm_digest.h): the launch sequence, the call that runs it behind a
// decode on the context's own workspace, and the host arithmetic that joins two digests.
#pragma once
#include <vector>

#include "mlp_ctx.h"
#include "pcm_digest.h"

// tiles the flat list can hold for n streams of max_total_bytes in all: every stream has at most one ragged tile
static inline uint64_t crc_max_tiles(uint32_t n, uint64_t max_total_bytes)
{
    return max_total_bytes / crc::TILE + n;
}

// workspace (uint32 words): tiles per stream [n + 1] | their exclusive scan [n + 1] | block sums of the scan | tile values
extern "C" size_t dvda_pcm_hip_crc32_workspace_words(uint32_t n, uint64_t max_total_bytes)
{
    return 2 * ((size_t)n + 1) + ((size_t)n + 1023) / 1024 + 2 + (size_t)crc_max_tiles(n, max_total_bytes);
}

extern "C" int dvda_pcm_hip_crc32(const int32_t *d_pcm, uint32_t layout, unsigned bits, const dvda_pcm_crc_desc *d_desc,
                                  uint32_t n, uint64_t max_total_bytes, uint32_t *d_crc, uint64_t *d_nbytes,
                                  uint32_t *d_work, size_t work_words, void *stream_)
{
    if (!d_pcm || !d_desc || !d_crc || !d_nbytes || !d_work || layout > DVDA_PCM_WAV16 || (bits != 16 && bits != 24) ||
        (layout == DVDA_PCM_WAV24 && bits != 24) || (layout == DVDA_PCM_WAV16 && bits != 16))
        return DVDA_HIP_EINVAL;
    if (work_words < dvda_pcm_hip_crc32_workspace_words(n, max_total_bytes))
        return DVDA_HIP_EINVAL;
    const uint64_t max_tiles = crc_max_tiles(n, max_total_bytes);
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
    uint32_t *tile_val = tmp + (n + 1023) / 1024 + 2;
    const uint32_t nb = bits / 8;
    hipLaunchKernelGGL(crc::k_crc_plan, dim3((n + 255) / 256), dim3(256), 0, st, d_desc, n, nb, cnt);
    enqueue_exscan(st, cnt, base, tmp, n, nullptr, n);
    const dim3 grid((unsigned)(max_tiles < crc::TILE_BLOCKS ? max_tiles : crc::TILE_BLOCKS)), block(crc::THREADS);
    if (layout == DVDA_PCM_PLANAR)
        hipLaunchKernelGGL(crc::k_crc_tiles<crc::SRC_PLANAR>, grid, block, 0, st, d_pcm, d_desc, n, nb, base, tile_val,
                           (uint32_t)max_tiles);
    else if (layout == DVDA_PCM_INTERLEAVED)
        hipLaunchKernelGGL(crc::k_crc_tiles<crc::SRC_FRAME_MAJOR>, grid, block, 0, st, d_pcm, d_desc, n, nb, base, tile_val,
                           (uint32_t)max_tiles);
    else
        hipLaunchKernelGGL(crc::k_crc_tiles<crc::SRC_WAV>, grid, block, 0, st, d_pcm, d_desc, n, nb, base, tile_val,
                           (uint32_t)max_tiles);
    hipLaunchKernelGGL(crc::k_crc_join, dim3(n), block, 0, st, d_desc, n, nb, base, tile_val, (uint32_t)max_tiles, d_crc,
                       d_nbytes);
    HIP_TRY(hipGetLastError());
    return DVDA_HIP_OK;
}

extern "C" int dvda_mlp_hip_pcm_crc32(dvda_mlp_hip_ctx *c, const int32_t *d_pcm, const uint64_t *d_out_off,
                                      const uint64_t *d_out_stride, unsigned bits, uint32_t *host_crc,
                                      uint64_t *host_nbytes, uint32_t n, void *stream_)
{
    if (!c || !d_pcm || !d_out_off || !d_out_stride || !host_crc || !host_nbytes)
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
        total += d.frames * d.channels * (bits / 8);
    }
    const size_t words = dvda_pcm_hip_crc32_workspace_words(n, total);
    if ((rc = c->d_crc_desc.grow(n)) != 0 || (rc = c->d_crc_out.grow(n)) != 0 || (rc = c->d_crc_bytes.grow(n)) != 0 ||
        (rc = c->d_crc_work.grow(words)) != 0)
        return rc;
    HIP_TRY(hipMemcpy(c->d_crc_desc, desc.data(), (size_t)n * sizeof(dvda_pcm_crc_desc), hipMemcpyHostToDevice));
    rc = dvda_pcm_hip_crc32(d_pcm, c->set.pcm_layout, bits, c->d_crc_desc, n, total, c->d_crc_out, c->d_crc_bytes,
                            c->d_crc_work, (size_t)c->d_crc_work.cap, stream_);
    if (rc)
        return rc;
    HIP_TRY(hipMemcpyAsync(host_crc, c->d_crc_out, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(host_nbytes, c->d_crc_bytes, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DVDA_HIP_OK;
}

extern "C" uint32_t dvda_pcm_hip_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b)
{
    // x has order 2^32 - 1 in the field, and 8 * len_b must not wrap: reduce the exponent first
    const uint64_t e = ((len_b % 0xFFFFFFFFull) * 8u) % 0xFFFFFFFFull;
    return crc::gfmul(crc_a, crc::xpow(e)) ^ crc_b;
}
