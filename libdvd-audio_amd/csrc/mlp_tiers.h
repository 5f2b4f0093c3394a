// mlp_tiers.h -- launchers of the tiers beside the MLP decode: raw-PCM sectors, the MLP track demux and the WAV
// payload.  No context: the caller brings the workspace.
#pragma once
#include "mlp_ctx.h"
#include "pcm_unswizzle.h"
#include "wav_pack.h"

// ------------------------------------------------------------------ PCM tier
// workspace (uint32 words): sec_frames[n] | sec_base[n + 1] | block sums[n / 1024 + 2] | n_bad
extern "C" size_t dvda_pcm_hip_workspace_words(uint32_t n_sectors)
{
    return (size_t)n_sectors + (size_t)n_sectors + 1 + ((size_t)n_sectors + 1023) / 1024 + 2 + 1;
}

extern "C" int dvda_pcm_hip_decode_sectors(const uint8_t *d_sectors, uint32_t n_sectors,
                                           unsigned bits_per_sample, unsigned channels, int32_t *d_pcm,
                                           uint64_t stride, uint32_t *d_work, void *stream_)
{
    if (!d_sectors || !d_pcm || !d_work || n_sectors == 0 || channels < 1 || channels > 6 ||
        (bits_per_sample != 16 && bits_per_sample != 24) || ((uintptr_t)d_sectors & 15))
        return DVDA_HIP_EINVAL;
    hipStream_t st = (hipStream_t)stream_;
    uint32_t *sec_frames = d_work;
    uint32_t *sec_base = d_work + n_sectors;
    uint32_t *tmp = sec_base + n_sectors + 1;
    const uint32_t blocks = (n_sectors + 1023) / 1024;
    uint32_t *n_bad = tmp + blocks + 2;
    const uint32_t chunk = (bits_per_sample / 8) * channels * 2;
    HIP_TRY(hipMemsetAsync(n_bad, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(pcm::k_pcm_scan, dim3((n_sectors + 255) / 256), dim3(256), 0, st, d_sectors, n_sectors,
                       chunk, sec_frames, n_bad);
    enqueue_exscan(st, sec_frames, sec_base, tmp, n_sectors, nullptr, n_sectors);
    {
        const dim3 g((n_sectors + 3) / 4), b(256);
#define DVDA_PCM_CASE(CH, NB)                                                                                  \
    case (CH) * 10 + (NB):                                                                                     \
        hipLaunchKernelGGL((pcm::k_pcm_unswizzle_t<CH, NB>), g, b, 0, st, d_sectors, n_sectors, sec_base, d_pcm, stride); \
        break;
        switch (channels * 10 + bits_per_sample / 8) {
            DVDA_PCM_CASE(1, 2) DVDA_PCM_CASE(2, 2) DVDA_PCM_CASE(3, 2) DVDA_PCM_CASE(4, 2) DVDA_PCM_CASE(5, 2)
            DVDA_PCM_CASE(6, 2) DVDA_PCM_CASE(1, 3) DVDA_PCM_CASE(2, 3) DVDA_PCM_CASE(3, 3) DVDA_PCM_CASE(4, 3)
            DVDA_PCM_CASE(5, 3) DVDA_PCM_CASE(6, 3)
        }
#undef DVDA_PCM_CASE
    }
    HIP_TRY(hipGetLastError());
    return DVDA_HIP_OK;
}

extern "C" int dvda_pcm_hip_result(const uint32_t *d_work, uint32_t n_sectors, uint64_t *pcm_frames,
                                   uint32_t *bad_sectors, void *stream_)
{
    if (!d_work || !pcm_frames)
        return DVDA_HIP_EINVAL;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream_));
    uint32_t total = 0, bad = 0;
    const uint32_t blocks = (n_sectors + 1023) / 1024;
    HIP_TRY(hipMemcpy(&total, d_work + n_sectors + n_sectors, sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&bad, d_work + n_sectors + n_sectors + 1 + blocks + 2, sizeof(uint32_t),
                      hipMemcpyDeviceToHost));
    *pcm_frames = total;
    if (bad_sectors)
        *bad_sectors = bad;
    return DVDA_HIP_OK;
}

// ------------------------------------------------------------------ MLP track demux
extern "C" int dvda_mlp_hip_demux_sectors(const uint8_t *d_sectors, uint32_t n_sectors, uint8_t *d_mlp,
                                          uint64_t mlp_cap, uint32_t *d_work, void *stream_)
{
    if (!d_sectors || !d_mlp || !d_work || n_sectors == 0 || ((uintptr_t)d_sectors & 15) || ((uintptr_t)d_mlp & 3))
        return DVDA_HIP_EINVAL;
    hipStream_t st = (hipStream_t)stream_;
    uint32_t *sec_bytes = d_work;
    uint32_t *sec_base = d_work + n_sectors;
    uint32_t *tmp = sec_base + n_sectors + 1;
    const uint32_t blocks = (n_sectors + 1023) / 1024;
    uint32_t *n_bad = tmp + blocks + 2;
    HIP_TRY(hipMemsetAsync(n_bad, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(pcm::k_mlp_sector_scan, dim3((n_sectors + 255) / 256), dim3(256), 0, st, d_sectors,
                       n_sectors, sec_bytes, n_bad);
    enqueue_exscan(st, sec_bytes, sec_base, tmp, n_sectors, nullptr, n_sectors);
    hipLaunchKernelGGL(pcm::k_mlp_gather, dim3((n_sectors + 3) / 4), dim3(256), 0, st, d_sectors, n_sectors,
                       sec_base, d_mlp, mlp_cap);
    HIP_TRY(hipGetLastError());
    return DVDA_HIP_OK;
}

// ------------------------------------------------------------------ WAV payload
extern "C" int dvda_mlp_hip_pack_wav(const int32_t *d_pcm, uint64_t stride, unsigned channels, uint64_t frames,
                                     unsigned bits_per_sample, uint8_t *d_out, void *stream_)
{
    if (!d_pcm || !d_out || channels < 1 || channels > 6 || (bits_per_sample != 16 && bits_per_sample != 24))
        return DVDA_HIP_EINVAL;
    if (frames == 0)
        return DVDA_HIP_OK;
    hipStream_t st = (hipStream_t)stream_;
    // whole 1024-frame blocks take the register-packing kernel when the planes and the output are
    // dword / 16-byte aligned; the tail (and unaligned buffers) the generic one
    uint64_t done = 0;
    const bool fast_ok = ((uintptr_t)d_pcm & 15) == 0 && (stride & 3) == 0 && ((uintptr_t)d_out & 3) == 0;
    const uint64_t nfast = fast_ok ? frames / wav::FAST_FRAMES : 0;
    if (nfast) {
        const dim3 g((unsigned)nfast), b(256);
#define DVDA_PACK_CASE(CH, BITS)                                                                        \
    case (CH) * 100 + (BITS):                                                                           \
        hipLaunchKernelGGL((wav::k_pack_wav_fast<CH, BITS>), g, b, 0, st, d_pcm, stride, nfast, d_out); \
        break;
        switch (channels * 100 + bits_per_sample) {
            DVDA_PACK_CASE(1, 16) DVDA_PACK_CASE(2, 16) DVDA_PACK_CASE(3, 16) DVDA_PACK_CASE(4, 16)
            DVDA_PACK_CASE(5, 16) DVDA_PACK_CASE(6, 16) DVDA_PACK_CASE(1, 24) DVDA_PACK_CASE(2, 24)
            DVDA_PACK_CASE(3, 24) DVDA_PACK_CASE(4, 24) DVDA_PACK_CASE(5, 24) DVDA_PACK_CASE(6, 24)
        }
#undef DVDA_PACK_CASE
        done = nfast * wav::FAST_FRAMES;
    }
    if (done < frames) {
        const uint64_t rest = frames - done;
        const uint64_t blocks = (rest + wav::FRAMES - 1) / wav::FRAMES;
        hipLaunchKernelGGL(wav::k_pack_wav, dim3((unsigned)blocks), dim3(256), 0, st, d_pcm + done, stride, channels,
                           rest, bits_per_sample, d_out + done * channels * (bits_per_sample / 8));
    }
    HIP_TRY(hipGetLastError());
    return DVDA_HIP_OK;
}
