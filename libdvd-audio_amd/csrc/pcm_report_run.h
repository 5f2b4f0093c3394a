// pcm_report_run.h -- host side of the eight passes over decoded PCM (pcm_digest.h, pcm_levels.h, pcm_compare.h, pcm_energy.h,
// pcm_requant.h, pcm_decim.h, pcm_resample.h, pcm_mix.h): what a report is to the driver (the three writers with an
// output buffer of their own on one base, WriterOut), the one driver of the flat tile list (pcm_tiles.h), the one call
// that runs a report behind a decode on the context's buffers, and the host arithmetic that joins two pieces' results.
#pragma once
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "mlp_ctx.h"
#include "pcm_compare.h"
#include "pcm_decim.h"
#include "pcm_digest.h"
#include "pcm_energy.h"
#include "pcm_levels.h"
#include "pcm_mix.h"
#include "pcm_requant.h"
#include "pcm_resample.h"

static inline bool int32_layout(uint32_t layout) { return layout == DVDA_PCM_PLANAR || layout == DVDA_PCM_INTERLEAVED; }

// the <IN_PLANAR, OUT_PLANAR> instance of a kernel template for two int32 layouts: pick(in, out) names the instance of
// the two constants' values
template <class Pick>
static inline auto planar_instance(uint32_t layout_in, uint32_t layout_out, Pick pick)
{
    const bool pi = layout_in == DVDA_PCM_PLANAR, po = layout_out == DVDA_PCM_PLANAR;
    return pi ? (po ? pick(std::true_type(), std::true_type()) : pick(std::true_type(), std::false_type()))
              : (po ? pick(std::false_type(), std::true_type()) : pick(std::false_type(), std::false_type()));
}

// What a report behind a decode lays into the context's buffers (report_of_decode, below), as its stage() states it on
// the host: the uint64 words it wants in d_rep_out -- its results first; none: nothing to run -- and what is uploaded
// into the last of them.
using Descs = std::vector<dvda_pcm_crc_desc>;
struct ReportStage {
    size_t out_words = 0;
    std::vector<uint64_t> behind;

    int want(size_t words)
    {
        out_words = words;
        return DVDA_HIP_OK;
    }
};

// ---- a report, as the driver sees it: the unit its tiles are cut in and the words a tile leaves in the workspace, the
//      layouts and depths it takes, where its results go, and its three launches.  Behind a decode it also states
//        units(d, bits)       what a descriptor adds to the bound on its list;
//        stage(desc, n, &s)   on the host: `s`; descriptors of its own behind the n of `desc` (uploaded with them); a
//                             verdict of its own as the return code;
//        bind(...)            on the device: where its results, what it staged and the descriptors lie.
//      What a report needs of the host for that travels in its last members ("(host)": the driver never reads them).
struct CrcReport {
    static constexpr uint32_t TILE = crc::TILE, TILE_WORDS = 1, TILE_BLOCKS = crc::TILE_BLOCKS;    // unit: payload bytes
    uint32_t *d_crc;
    uint64_t *d_nbytes;

    bool has_out() const { return d_crc && d_nbytes; }
    static bool takes(uint32_t layout, unsigned bits)
    {
        return layout <= DVDA_PCM_WAV16 && (bits == 16 || bits == 24) && !(layout == DVDA_PCM_WAV24 && bits != 24) &&
               !(layout == DVDA_PCM_WAV16 && bits != 16);
    }
    uint64_t units(const dvda_pcm_crc_desc &d, unsigned bits) const { return d.frames * d.channels * (bits / 8); }
    // the results of n streams in one block of uint64 words: the byte counts, then the digests
    int stage(Descs &, uint32_t n, ReportStage *s) const { return s->want(n + ((size_t)n + 1) / 2); }
    void bind(uint64_t *d_out, uint64_t *, const dvda_pcm_crc_desc *, uint32_t n) { *this = {(uint32_t *)(d_out + n), d_out}; }

    void plan(hipStream_t st, const dvda_pcm_crc_desc *d_desc, uint32_t n, unsigned bits, uint32_t *cnt) const
    {
        hipLaunchKernelGGL(crc::k_crc_plan, dim3((n + 255) / 256), dim3(256), 0, st, d_desc, n, bits / 8, cnt);
    }
    void tiles(dim3 grid, dim3 block, hipStream_t st, const int32_t *d_pcm, uint32_t layout, const dvda_pcm_crc_desc *d_desc,
               uint32_t n, unsigned bits, const uint32_t *base, uint32_t *tile_val, uint32_t max_tiles) const
    {
        const uint32_t nb = bits / 8;
        if (layout == DVDA_PCM_PLANAR)
            hipLaunchKernelGGL(crc::k_crc_tiles<crc::SRC_PLANAR>, grid, block, 0, st, d_pcm, d_desc, n, nb, base, tile_val,
                               max_tiles);
        else if (layout == DVDA_PCM_INTERLEAVED)
            hipLaunchKernelGGL(crc::k_crc_tiles<crc::SRC_FRAME_MAJOR>, grid, block, 0, st, d_pcm, d_desc, n, nb, base,
                               tile_val, max_tiles);
        else
            hipLaunchKernelGGL(crc::k_crc_tiles<crc::SRC_WAV>, grid, block, 0, st, d_pcm, d_desc, n, nb, base, tile_val,
                               max_tiles);
    }
    void join(dim3 block, hipStream_t st, const dvda_pcm_crc_desc *d_desc, uint32_t n, unsigned bits, const uint32_t *base,
              const uint32_t *tile_val, uint32_t max_tiles) const
    {
        hipLaunchKernelGGL(crc::k_crc_join, dim3(n), block, 0, st, d_desc, n, bits / 8, base, tile_val, max_tiles, d_crc,
                           d_nbytes);
    }
};

struct LvlReport {
    static constexpr uint32_t TILE = lvl::TILE, TILE_WORDS = lvl::REC, TILE_BLOCKS = lvl::TILE_BLOCKS;     // unit: frames
    dvda_pcm_levels *d_levels;

    bool has_out() const { return d_levels != nullptr; }
    static bool takes(uint32_t layout, unsigned bits) { return (bits == 16 || bits == 20 || bits == 24) && int32_layout(layout); }
    uint64_t units(const dvda_pcm_crc_desc &d, unsigned) const { return d.frames; }
    int stage(Descs &, uint32_t n, ReportStage *s) const { return s->want((size_t)n * (sizeof(dvda_pcm_levels) / 8)); }
    void bind(uint64_t *d_out, uint64_t *, const dvda_pcm_crc_desc *, uint32_t) { d_levels = (dvda_pcm_levels *)d_out; }

    void plan(hipStream_t st, const dvda_pcm_crc_desc *d_desc, uint32_t n, unsigned, uint32_t *cnt) const
    {
        hipLaunchKernelGGL(lvl::k_lvl_plan, dim3((n + 255) / 256), dim3(256), 0, st, d_desc, n, cnt);
    }
    void tiles(dim3 grid, dim3 block, hipStream_t st, const int32_t *d_pcm, uint32_t layout, const dvda_pcm_crc_desc *d_desc,
               uint32_t n, unsigned bits, const uint32_t *base, uint32_t *rec, uint32_t max_tiles) const
    {
        if (layout == DVDA_PCM_PLANAR)
            hipLaunchKernelGGL(lvl::k_lvl_tiles<true>, grid, block, 0, st, d_pcm, d_desc, n, (uint32_t)bits, base, rec,
                               max_tiles);
        else
            hipLaunchKernelGGL(lvl::k_lvl_tiles<false>, grid, block, 0, st, d_pcm, d_desc, n, (uint32_t)bits, base, rec,
                               max_tiles);
    }
    void join(dim3 block, hipStream_t st, const dvda_pcm_crc_desc *d_desc, uint32_t n, unsigned, const uint32_t *base,
              const uint32_t *rec, uint32_t max_tiles) const
    {
        hipLaunchKernelGGL(lvl::k_lvl_join, dim3(n), block, 0, st, d_desc, n, base, rec, max_tiles, d_levels);
    }
};
static_assert(sizeof(dvda_pcm_levels) % sizeof(uint64_t) == 0, "reports lie in a block of uint64 words");

// The compare: side A is what the driver calls the PCM; side B -- buffer, layout, descriptors -- travels here.
struct CmpReport {
    static constexpr uint32_t TILE = cmp::TILE, TILE_WORDS = cmp::REC, TILE_BLOCKS = cmp::TILE_BLOCKS;     // unit: frames
    dvda_pcm_diff *d_diff;
    const int32_t *d_b;
    uint32_t layout_b;
    const dvda_pcm_crc_desc *d_desc_b;

    bool has_out() const { return d_diff && d_b && d_desc_b && int32_layout(layout_b); }
    static bool takes(uint32_t layout, unsigned bits)
    {
        return (bits == 0 || bits == 16 || bits == 20 || bits == 24) && int32_layout(layout);
    }
    // (side A's frames: at least what the pair compares)
    uint64_t units(const dvda_pcm_crc_desc &d, unsigned) const { return d.frames; }
    int stage(Descs &, uint32_t n, ReportStage *s) const { return s->want((size_t)n * (sizeof(dvda_pcm_diff) / 8)); }
    void bind(uint64_t *d_out, uint64_t *, const dvda_pcm_crc_desc *, uint32_t) { d_diff = (dvda_pcm_diff *)d_out; }

    void plan(hipStream_t st, const dvda_pcm_crc_desc *d_desc, uint32_t n, unsigned, uint32_t *cnt) const
    {
        hipLaunchKernelGGL(cmp::k_cmp_plan, dim3((n + 255) / 256), dim3(256), 0, st, d_desc, d_desc_b, n, cnt);
    }
    void tiles(dim3 grid, dim3 block, hipStream_t st, const int32_t *d_a, uint32_t layout, const dvda_pcm_crc_desc *d_desc,
               uint32_t n, unsigned bits, const uint32_t *base, uint32_t *rec, uint32_t max_tiles) const
    {
        auto k = planar_instance(layout, layout_b, [](auto a, auto b) { return cmp::k_cmp_tiles<a.value, b.value>; });
        hipLaunchKernelGGL(k, grid, block, 0, st, d_a, d_desc, d_b, d_desc_b, n, (uint32_t)bits, base, rec, max_tiles);
    }
    void join(dim3 block, hipStream_t st, const dvda_pcm_crc_desc *d_desc, uint32_t n, unsigned, const uint32_t *base,
              const uint32_t *rec, uint32_t max_tiles) const
    {
        hipLaunchKernelGGL(cmp::k_cmp_join, dim3(n), block, 0, st, d_desc, d_desc_b, n, base, rec, max_tiles, d_diff);
    }
};
static_assert(sizeof(dvda_pcm_diff) == 160, "dvda_pcm_diff is 160 bytes");

// The energy report: its unit is a piece of a block, so the grid -- B, the leads -- travels here with the four outputs,
// and the bound on its list is its own.
struct NrgReport {
    static constexpr uint32_t TILE = nrg::PIECE, TILE_WORDS = nrg::REC, TILE_BLOCKS = nrg::TILE_BLOCKS;    // unit: frames
    uint32_t block_frames;
    const uint32_t *d_lead;
    dvda_pcm_energy_block *d_blocks;
    const uint64_t *d_block_off, *d_block_cap;
    uint64_t *d_nblocks;
    uint64_t cap_blocks;            // (host) the blocks the caller has room for, and where it is told each stream's first
    uint64_t *host_first;

    static bool block_ok(uint32_t b) { return b >= DVDA_NRG_MIN_BLOCK && b <= DVDA_NRG_MAX_BLOCK; }
    bool has_out() const { return block_ok(block_frames) && d_blocks && d_block_off && d_block_cap && d_nblocks; }
    static bool takes(uint32_t layout, unsigned) { return int32_layout(layout); }
    // every block has at most one ragged piece, and a stream at most frames / B + 2 blocks
    uint64_t max_tiles(uint32_t n, uint64_t max_total) const
    {
        return max_total / nrg::PIECE + max_total / block_frames + 2ull * n;
    }
    uint64_t units(const dvda_pcm_crc_desc &d, unsigned) const { return PCMT_NOT_TAKEN(d) ? 0 : d.frames; }
    // The streams back to back: what each needs is known on the host (every grid starts at its stream's first frame), so
    // the verdict falls here: host_first is filled, or ECAPACITY carries the count in host_first[n], and no blocks is OK.
    // d_rep_out: the blocks (21 words each) | off [n] | cap [n] | nblocks [n]
    int stage(Descs &desc, uint32_t n, ReportStage *s) const
    {
        std::vector<uint64_t> first((size_t)n + 1);
        for (uint32_t i = 0; i < n; i++)
            first[i + 1] = first[i] + nrg::grid_of(desc[i], block_frames, block_frames).blocks();
        if (first[n] > cap_blocks) {
            host_first[n] = first[n];
            return DVDA_HIP_ECAPACITY;
        }
        std::copy(first.begin(), first.end(), host_first);
        s->behind = std::vector<uint64_t>(3 * (size_t)n);
        for (uint32_t i = 0; i < n; i++) {
            s->behind[i] = first[i];
            s->behind[n + i] = first[i + 1] - first[i];
        }
        return s->want(first[n] ? first[n] * (sizeof(dvda_pcm_energy_block) / 8) + 3 * (uint64_t)n : 0);
    }
    void bind(uint64_t *d_out, uint64_t *d_behind, const dvda_pcm_crc_desc *, uint32_t n)
    {
        d_blocks = (dvda_pcm_energy_block *)d_out;
        d_block_off = d_behind;
        d_block_cap = d_behind + n;
        d_nblocks = d_behind + 2 * (size_t)n;
    }

    void plan(hipStream_t st, const dvda_pcm_crc_desc *d_desc, uint32_t n, unsigned, uint32_t *cnt) const
    {
        hipLaunchKernelGGL(nrg::k_nrg_plan, dim3((n + 255) / 256), dim3(256), 0, st, d_desc, n, block_frames, d_lead, cnt);
    }
    void tiles(dim3 grid, dim3 block, hipStream_t st, const int32_t *d_pcm, uint32_t layout, const dvda_pcm_crc_desc *d_desc,
               uint32_t n, unsigned, const uint32_t *base, uint32_t *rec, uint32_t max_tiles) const
    {
        if (layout == DVDA_PCM_PLANAR)
            hipLaunchKernelGGL(nrg::k_nrg_tiles<true>, grid, block, 0, st, d_pcm, d_desc, n, block_frames, d_lead, base, rec,
                               max_tiles);
        else
            hipLaunchKernelGGL(nrg::k_nrg_tiles<false>, grid, block, 0, st, d_pcm, d_desc, n, block_frames, d_lead, base, rec,
                               max_tiles);
    }
    void join(dim3 block, hipStream_t st, const dvda_pcm_crc_desc *d_desc, uint32_t n, unsigned, const uint32_t *base,
              const uint32_t *rec, uint32_t max_tiles) const
    {
        hipLaunchKernelGGL(nrg::k_nrg_join, dim3(n), block, 0, st, d_desc, n, block_frames, d_lead, base, rec, max_tiles,
                           d_blocks, d_block_off, d_block_cap, d_nblocks);
    }
};
static_assert(sizeof(dvda_pcm_energy_block) == 168, "dvda_pcm_energy_block is 168 bytes");

// The word-length reduction: the one report that also writes PCM.  The input is what the driver calls the PCM; the
// output -- buffer, layout, descriptors -- the streams' first absolute frames and the parameters travel here.
struct RqReport {
    static constexpr uint32_t TILE = rq::TILE, TILE_WORDS = rq::REC, TILE_BLOCKS = rq::TILE_BLOCKS;        // unit: frames
    dvda_pcm_requant_report *d_report;
    int32_t *d_out;
    uint32_t layout_out;
    const dvda_pcm_crc_desc *d_desc_out;
    const uint64_t *d_frame0;
    const dvda_pcm_requant *params;         // (host)
    const uint64_t *host_frame0;            // (host) behind a decode: the streams' first frames, or none

    uint64_t units(const dvda_pcm_crc_desc &d, unsigned) const { return PCMT_NOT_TAKEN(d) ? 0 : d.frames; }
    // d_rep_out: the reports (9 words each) | frame0 [n]; in place: the output's descriptors are the input's
    int stage(Descs &, uint32_t n, ReportStage *s) const
    {
        if (host_frame0)
            s->behind.assign(host_frame0, host_frame0 + n);
        return s->want((sizeof(dvda_pcm_requant_report) / 8 + 1) * (size_t)n);
    }
    void bind(uint64_t *d_out_, uint64_t *d_behind, const dvda_pcm_crc_desc *d_desc, uint32_t)
    {
        d_report = (dvda_pcm_requant_report *)d_out_;
        d_desc_out = d_desc;
        d_frame0 = d_behind;
    }
    bool layout_out_ok() const
    {
        return int32_layout(layout_out) || (layout_out == DVDA_PCM_WAV16 && params->bits_out == 16) ||
               (layout_out == DVDA_PCM_WAV24 && params->bits_out == 24);
    }
    bool has_out() const { return d_report && d_out && d_desc_out && params && rq::params_ok(*params) && layout_out_ok(); }
    static bool takes(uint32_t layout, unsigned) { return int32_layout(layout); }

    void plan(hipStream_t st, const dvda_pcm_crc_desc *d_desc, uint32_t n, unsigned, uint32_t *cnt) const
    {
        hipLaunchKernelGGL(rq::k_rq_plan, dim3((n + 255) / 256), dim3(256), 0, st, d_desc, d_desc_out, n, cnt);
    }
    template <bool IN_PLANAR>
    void tiles_in(dim3 grid, dim3 block, hipStream_t st, const int32_t *d_pcm, const dvda_pcm_crc_desc *d_desc, uint32_t n,
                  const uint32_t *base, uint32_t *rec, uint32_t max_tiles) const
    {
        auto k = layout_out == DVDA_PCM_PLANAR        ? rq::k_rq_tiles<IN_PLANAR, rq::OUT_PLANAR>
                 : layout_out == DVDA_PCM_INTERLEAVED ? rq::k_rq_tiles<IN_PLANAR, rq::OUT_FRAME_MAJOR>
                 : layout_out == DVDA_PCM_WAV24       ? rq::k_rq_tiles<IN_PLANAR, rq::OUT_WAV24>
                                                      : rq::k_rq_tiles<IN_PLANAR, rq::OUT_WAV16>;
        hipLaunchKernelGGL(k, grid, block, 0, st, d_pcm, d_desc, d_out, d_desc_out, d_frame0, n, rq::par_of(*params), base,
                           rec, max_tiles);
    }
    void tiles(dim3 grid, dim3 block, hipStream_t st, const int32_t *d_pcm, uint32_t layout, const dvda_pcm_crc_desc *d_desc,
               uint32_t n, unsigned, const uint32_t *base, uint32_t *rec, uint32_t max_tiles) const
    {
        if (layout == DVDA_PCM_PLANAR)
            tiles_in<true>(grid, block, st, d_pcm, d_desc, n, base, rec, max_tiles);
        else
            tiles_in<false>(grid, block, st, d_pcm, d_desc, n, base, rec, max_tiles);
    }
    void join(dim3 block, hipStream_t st, const dvda_pcm_crc_desc *d_desc, uint32_t n, unsigned, const uint32_t *base,
              const uint32_t *rec, uint32_t max_tiles) const
    {
        hipLaunchKernelGGL(rq::k_rq_join, dim3(n), block, 0, st, d_desc, d_desc_out, n, base, rec, max_tiles, d_report);
    }
};
static_assert(sizeof(dvda_pcm_requant) == 24 && sizeof(dvda_pcm_requant_report) == 72, "the requantizer's structs");

// What the writers that lay their output into a buffer of its own (decimate, resample, mix) share: the input is what
// the driver calls the PCM; the output -- buffer, layout, descriptors -- and the results travel here, and behind a decode
// where the output's regions lie.
template <class Rep>
struct WriterOut {
    Rep *d_report;
    int32_t *d_out;
    uint32_t layout_out;
    const dvda_pcm_crc_desc *d_desc_out;
    const uint64_t *host_off, *host_stride;     // (host) behind a decode: where the output's regions lie

    bool out_ok() const { return d_report && d_out && d_desc_out && int32_layout(layout_out); }
    // the descriptors of both sides in one array: the input's [n], then the output's [n] -- the input's at the output's
    // place, shape(o, i) making the frames and channels the output's.  d_rep_out: the reports | s->behind -- so a pass
    // that lays words behind its reports (the mix's matrices) fills s->behind BEFORE it calls this, and `s` is the fresh
    // one of this call (report_of_decode makes it): the words wanted are counted from what it holds here
    template <class Shape>
    int stage_out(Descs &desc, uint32_t n, ReportStage *s, Shape shape) const
    {
        desc.resize(2 * (size_t)n);
        for (uint32_t i = 0; i < n; i++) {
            dvda_pcm_crc_desc &o = desc[n + i];
            o = desc[i];
            o.off = host_off[i];
            o.stride = host_stride[i];
            shape(o, i);
        }
        return s->want((size_t)n * (sizeof(Rep) / 8) + s->behind.size());
    }
    void bind(uint64_t *d_out_, uint64_t *, const dvda_pcm_crc_desc *d_desc, uint32_t n)
    {
        d_report = (Rep *)d_out_;
        d_desc_out = d_desc + n;
    }
};

// The decimation: the pieces and the ratio travel here.  Its unit is OUTPUT frames; the driver's `bits` is the depth the
// values are clamped to.
struct DcReport : WriterOut<dvda_pcm_decim_report> {
    static constexpr uint32_t TILE = dcm::TILE, TILE_WORDS = dcm::REC, TILE_BLOCKS = dcm::TILE_BLOCKS;     // unit: output frames
    const dvda_pcm_decim_piece *d_piece;
    uint32_t ratio;

    // (an overflowed stream has no frames here: zeros reported, nothing written)
    uint64_t units(const dvda_pcm_crc_desc &d, unsigned) const
    {
        return PCMT_NOT_TAKEN(d) ? 0 : dcm::out_frames(0, d.frames, ratio);
    }
    int stage(Descs &desc, uint32_t n, ReportStage *s) const
    {
        return stage_out(desc, n, s, [&](dvda_pcm_crc_desc &o, uint32_t) { o.frames = units(o, 0); });
    }
    bool has_out() const { return out_ok() && dcm::ratio_ok(ratio); }
    static bool takes(uint32_t layout, unsigned bits) { return int32_layout(layout) && dcm::depth_ok(bits); }

    void plan(hipStream_t st, const dvda_pcm_crc_desc *d_desc, uint32_t n, unsigned, uint32_t *cnt) const
    {
        hipLaunchKernelGGL(dcm::k_dc_plan, dim3((n + 255) / 256), dim3(256), 0, st, d_desc, d_desc_out, d_piece, n, ratio, cnt);
    }
    template <uint32_t D>
    void tiles_of(dim3 grid, dim3 block, hipStream_t st, const int32_t *d_pcm, uint32_t layout, const dvda_pcm_crc_desc *d_desc,
                  uint32_t n, unsigned bits, const uint32_t *base, uint32_t *rec, uint32_t max_tiles) const
    {
        auto k = planar_instance(layout, layout_out, [](auto i, auto o) { return dcm::k_dc_tiles<D, i.value, o.value>; });
        hipLaunchKernelGGL(k, grid, block, 0, st, d_pcm, d_desc, d_out, d_desc_out, d_piece, n, (uint32_t)bits, base, rec,
                           max_tiles);
    }
    void tiles(dim3 grid, dim3 block, hipStream_t st, const int32_t *d_pcm, uint32_t layout, const dvda_pcm_crc_desc *d_desc,
               uint32_t n, unsigned bits, const uint32_t *base, uint32_t *rec, uint32_t max_tiles) const
    {
        if (ratio == 2)
            tiles_of<2>(grid, block, st, d_pcm, layout, d_desc, n, bits, base, rec, max_tiles);
        else
            tiles_of<4>(grid, block, st, d_pcm, layout, d_desc, n, bits, base, rec, max_tiles);
    }
    void join(dim3 block, hipStream_t st, const dvda_pcm_crc_desc *d_desc, uint32_t n, unsigned, const uint32_t *base,
              const uint32_t *rec, uint32_t max_tiles) const
    {
        hipLaunchKernelGGL(dcm::k_dc_join, dim3(n), block, 0, st, d_desc, d_desc_out, d_piece, n, ratio, base, rec, max_tiles,
                           d_report);
    }
};
static_assert(sizeof(dvda_pcm_decim_piece) == 16 && sizeof(dvda_pcm_decim_report) == 80, "the decimator's structs");

// The resampler, 48 kHz to 44.1 kHz: the decimator's shape without a ratio.
struct RsReport : WriterOut<dvda_pcm_decim_report> {
    static constexpr uint32_t TILE = rsm::TILE, TILE_WORDS = rsm::REC, TILE_BLOCKS = rsm::TILE_BLOCKS;     // unit: output frames
    const dvda_pcm_decim_piece *d_piece;

    // (an overflowed stream has no frames here: zeros reported, nothing written)
    uint64_t units(const dvda_pcm_crc_desc &d, unsigned) const { return PCMT_NOT_TAKEN(d) ? 0 : rsm::out_frames(0, d.frames); }
    int stage(Descs &desc, uint32_t n, ReportStage *s) const
    {
        return stage_out(desc, n, s, [&](dvda_pcm_crc_desc &o, uint32_t) { o.frames = units(o, 0); });
    }
    bool has_out() const { return out_ok(); }
    static bool takes(uint32_t layout, unsigned bits) { return int32_layout(layout) && rsm::depth_ok(bits); }

    void plan(hipStream_t st, const dvda_pcm_crc_desc *d_desc, uint32_t n, unsigned, uint32_t *cnt) const
    {
        hipLaunchKernelGGL(rsm::k_rs_plan, dim3((n + 255) / 256), dim3(256), 0, st, d_desc, d_desc_out, d_piece, n, cnt);
    }
    void tiles(dim3 grid, dim3 block, hipStream_t st, const int32_t *d_pcm, uint32_t layout, const dvda_pcm_crc_desc *d_desc,
               uint32_t n, unsigned bits, const uint32_t *base, uint32_t *rec, uint32_t max_tiles) const
    {
        auto k = planar_instance(layout, layout_out, [](auto i, auto o) { return rsm::k_rs_tiles<i.value, o.value>; });
        hipLaunchKernelGGL(k, grid, block, 0, st, d_pcm, d_desc, d_out, d_desc_out, d_piece, n, (uint32_t)bits, base, rec,
                           max_tiles);
    }
    void join(dim3 block, hipStream_t st, const dvda_pcm_crc_desc *d_desc, uint32_t n, unsigned, const uint32_t *base,
              const uint32_t *rec, uint32_t max_tiles) const
    {
        hipLaunchKernelGGL(rsm::k_rs_join, dim3(n), block, 0, st, d_desc, d_desc_out, d_piece, n, base, rec, max_tiles,
                           d_report);
    }
};

// The channel mix: the matrices (a device array, so the kernels judge them) travel here.  Its unit is frames; the
// driver's `bits` is the depth the values are clamped to.
struct MixReport : WriterOut<dvda_pcm_mix_report> {
    static constexpr uint32_t TILE = mix::TILE, TILE_WORDS = mix::REC, TILE_BLOCKS = mix::TILE_BLOCKS;     // unit: frames
    const dvda_pcm_mix *d_mix;
    const dvda_pcm_mix *host_mix;               // (host) behind a decode: the streams' matrices

    // (an overflowed stream has no frames here: zeros reported, nothing written)
    uint64_t units(const dvda_pcm_crc_desc &d, unsigned) const { return PCMT_NOT_TAKEN(d) ? 0 : d.frames; }
    // the output's descriptors say the matrix's output channels; the matrices (33 words each) lie behind the reports
    int stage(Descs &desc, uint32_t n, ReportStage *s) const
    {
        s->behind.resize(sizeof(dvda_pcm_mix) / 8 * n);
        memcpy(s->behind.data(), host_mix, sizeof(dvda_pcm_mix) * (size_t)n);
        return stage_out(desc, n, s, [&](dvda_pcm_crc_desc &o, uint32_t i) { o.channels = host_mix[i].out_channels; });
    }
    void bind(uint64_t *d_out_, uint64_t *d_behind, const dvda_pcm_crc_desc *d_desc, uint32_t n)
    {
        WriterOut::bind(d_out_, d_behind, d_desc, n);
        d_mix = (const dvda_pcm_mix *)d_behind;
    }
    bool has_out() const { return out_ok() && d_mix; }
    static bool takes(uint32_t layout, unsigned bits) { return int32_layout(layout) && mix::depth_ok(bits); }

    void plan(hipStream_t st, const dvda_pcm_crc_desc *d_desc, uint32_t n, unsigned, uint32_t *cnt) const
    {
        hipLaunchKernelGGL(mix::k_mix_plan, dim3((n + 255) / 256), dim3(256), 0, st, d_desc, d_desc_out, d_mix, n, cnt);
    }
    void tiles(dim3 grid, dim3 block, hipStream_t st, const int32_t *d_pcm, uint32_t layout, const dvda_pcm_crc_desc *d_desc,
               uint32_t n, unsigned bits, const uint32_t *base, uint32_t *rec, uint32_t max_tiles) const
    {
        auto k = planar_instance(layout, layout_out, [](auto i, auto o) { return mix::k_mix_tiles<i.value, o.value>; });
        hipLaunchKernelGGL(k, grid, block, 0, st, d_pcm, d_desc, d_out, d_desc_out, d_mix, n, (uint32_t)bits, base, rec,
                           max_tiles);
    }
    void join(dim3 block, hipStream_t st, const dvda_pcm_crc_desc *d_desc, uint32_t n, unsigned, const uint32_t *base,
              const uint32_t *rec, uint32_t max_tiles) const
    {
        hipLaunchKernelGGL(mix::k_mix_join, dim3(n), block, 0, st, d_desc, d_desc_out, d_mix, n, base, rec, max_tiles,
                           d_report);
    }
};
static_assert(sizeof(dvda_pcm_mix) == 264 && sizeof(dvda_pcm_mix_report) == 72, "the mix's structs");

// ---- the driver of the flat tile list
// tiles the list can hold for n streams of max_total units in all: every stream has at most one ragged tile -- unless the
// report `r` supplies its own bound, max_tiles(n, max_total), from what it carries (the energy report's pieces depend on
// its block length, and on nothing else of it)
template <class R>
static inline auto report_max_tiles(const R &r, uint32_t n, uint64_t max_total, int) -> decltype(r.max_tiles(n, max_total))
{
    return r.max_tiles(n, max_total);
}
template <class R>
static inline uint64_t report_max_tiles(const R &, uint32_t n, uint64_t max_total, long)
{
    return max_total / R::TILE + n;
}

// workspace (uint32 words): tiles per stream [n + 1] | their exclusive scan [n + 1] | block sums of the scan | what the
// tiles leave
template <class R>
static inline size_t report_workspace_words(const R &r, uint32_t n, uint64_t max_total)
{
    return 2 * ((size_t)n + 1) + ((size_t)n + 1023) / 1024 + 2 + (size_t)report_max_tiles(r, n, max_total, 0) * R::TILE_WORDS;
}

// (asked of the runtime once per process)
static bool report_have_device()
{
    static const bool have = [] {
        int ndev = 0;
        return hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
    }();
    return have;
}

// plan -> scan -> tiles -> join, enqueued on `stream_`.  The arguments are judged first, on any machine, then the device.
template <class R>
static int report_run(const R &r, const int32_t *d_pcm, uint32_t layout, unsigned bits, const dvda_pcm_crc_desc *d_desc,
                      uint32_t n, uint64_t max_total, uint32_t *d_work, size_t work_words, void *stream_)
{
    if (!d_pcm || !d_desc || !d_work || !r.has_out() || !R::takes(layout, bits))
        return DVDA_HIP_EINVAL;
    if (work_words < report_workspace_words(r, n, max_total))
        return DVDA_HIP_EINVAL;
    const uint64_t max_tiles = report_max_tiles(r, n, max_total, 0);
    if (max_tiles >> 31)
        return DVDA_HIP_ECAPACITY;
    if (!report_have_device())
        return DVDA_HIP_ENODEV;
    if (n == 0)
        return DVDA_HIP_OK;
    hipStream_t st = (hipStream_t)stream_;
    uint32_t *cnt = d_work;
    uint32_t *base = cnt + n + 1;
    uint32_t *tmp = base + n + 1;
    uint32_t *tile_out = tmp + (n + 1023) / 1024 + 2;
    r.plan(st, d_desc, n, bits, cnt);
    enqueue_exscan(st, cnt, base, tmp, n, nullptr, n);
    const dim3 grid((unsigned)(max_tiles < R::TILE_BLOCKS ? max_tiles : R::TILE_BLOCKS)), block(pcmt::THREADS);
    r.tiles(grid, block, st, d_pcm, layout, d_desc, n, bits, base, tile_out, (uint32_t)max_tiles);
    r.join(block, st, d_desc, n, bits, base, tile_out, (uint32_t)max_tiles);
    HIP_TRY(hipGetLastError());
    return DVDA_HIP_OK;
}

// n clamped to the batch of the context's last decode (0: nothing to do); ESTATE for a context that has not indexed
static int report_clamp(const dvda_mlp_hip_ctx *c, uint32_t *n_io)
{
    if (!c->indexed)
        return DVDA_HIP_ESTATE;
    if (*n_io > c->n_streams)
        *n_io = c->n_streams;
    return DVDA_HIP_OK;
}

// The descriptors of the first n (clamped to the batch; 0: nothing to do) streams of the context's last decode, on the
// host: frames and channels from what dvda_mlp_hip_stream_info says, off / stride from the caller's d_out_off /
// d_out_stride, copied down.  Blocks.
static int report_decode_descs(dvda_mlp_hip_ctx *c, const uint64_t *d_out_off, const uint64_t *d_out_stride, uint32_t *n_io,
                               void *stream_, std::vector<dvda_pcm_crc_desc> *desc_)
{
    int rc = report_clamp(c, n_io);
    const uint32_t n = *n_io;
    if (rc || n == 0)
        return rc;
    // frames and channels as the caller is told them: conceal mode's composed record and the presentation included
    std::vector<dvda_mlp_stream_info> infos(n);
    if ((rc = dvda_mlp_hip_stream_info(c, infos.data(), n, stream_)) != 0)
        return rc;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<uint64_t> off(n), stride(n);
    HIP_TRY(hipMemcpy(off.data(), d_out_off, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(stride.data(), d_out_stride, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    std::vector<dvda_pcm_crc_desc> &desc = *desc_;
    desc.resize(n);
    for (uint32_t i = 0; i < n; i++) {
        dvda_pcm_crc_desc &d = desc[i];
        d.off = off[i];
        d.stride = stride[i];
        // (an overflowed stream's region does not hold the stream)
        d.frames = (infos[i].status & DVDA_ST_OVERFLOW) ? 0 : infos[i].pcm_frames;
        d.channels = infos[i].channels;
        d.reserved = 0;
    }
    return DVDA_HIP_OK;
}

// The report of the first n (clamped to the batch; 0: nothing to do) streams of the context's last decode, on the
// context's buffers: the report's stage on the host, the buffers grown to it, the descriptors -- and what the report laid
// behind its results -- copied up, the report bound to where all of it lies, then its run, enqueued on `stream_`.  *r:
// where the results lie on the device; the caller copies them down and waits (report_down).  *n_io: 0 where there is
// nothing to copy down -- no streams, or a stage that wants no words.  Blocks for the descriptors.
template <class R>
static int report_of_decode(dvda_mlp_hip_ctx *c, const int32_t *d_pcm, const uint64_t *d_out_off,
                            const uint64_t *d_out_stride, unsigned bits, uint32_t *n_io, void *stream_, R *r)
{
    Descs desc;
    ReportStage s;
    int rc = report_decode_descs(c, d_out_off, d_out_stride, n_io, stream_, &desc);
    const uint32_t n = *n_io;
    if (rc || (rc = r->stage(desc, n, &s)) != 0 || s.out_words == 0) {
        *n_io = 0;
        return rc;
    }
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++)
        total += r->units(desc[i], bits);
    if ((rc = c->d_rep_desc.grow(desc.size())) != 0 || (rc = c->d_rep_out.grow(s.out_words)) != 0 ||
        (rc = c->d_rep_work.grow(report_workspace_words(*r, n, total))) != 0)
        return rc;
    uint64_t *d_behind = s.behind.empty() ? nullptr : c->d_rep_out + (s.out_words - s.behind.size());
    HIP_TRY(hipMemcpy(c->d_rep_desc, desc.data(), desc.size() * sizeof(dvda_pcm_crc_desc), hipMemcpyHostToDevice));
    if (d_behind)
        HIP_TRY(hipMemcpy(d_behind, s.behind.data(), s.behind.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    r->bind(c->d_rep_out, d_behind, c->d_rep_desc, n);
    return report_run(*r, d_pcm, c->set.pcm_layout, bits, c->d_rep_desc, n, total, c->d_rep_work,
                      (size_t)c->d_rep_work.cap, stream_);
}

// ... and the results copied down behind it on its stream (a second array where the report has two), and the wait
static int report_down(void *stream_, void *host, const void *dev, size_t bytes, void *host2 = nullptr,
                       const void *dev2 = nullptr, size_t bytes2 = 0)
{
    hipStream_t st = (hipStream_t)stream_;
    HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
    if (host2)
        HIP_TRY(hipMemcpyAsync(host2, dev2, bytes2, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DVDA_HIP_OK;
}

// What the *_value entry points do around their pass's value(): bad arguments (`ok` false) give 0 with *clipped = -1,
// else value(&cl) with *clipped = whether the clamp changed it.  clipped may be NULL.
template <class Value>
static inline int32_t value_or_bad(bool ok, int *clipped, Value value)
{
    uint32_t cl = 0;
    const int32_t y = ok ? value(&cl) : 0;
    if (clipped)
        *clipped = ok ? (int)cl : -1;
    return y;
}

// ---- the digest
extern "C" size_t dvda_pcm_hip_crc32_workspace_words(uint32_t n, uint64_t max_total_bytes)
{
    return report_workspace_words(CrcReport{}, n, max_total_bytes);
}

extern "C" int dvda_pcm_hip_crc32(const int32_t *d_pcm, uint32_t layout, unsigned bits, const dvda_pcm_crc_desc *d_desc,
                                  uint32_t n, uint64_t max_total_bytes, uint32_t *d_crc, uint64_t *d_nbytes,
                                  uint32_t *d_work, size_t work_words, void *stream_)
{
    return report_run(CrcReport{d_crc, d_nbytes}, d_pcm, layout, bits, d_desc, n, max_total_bytes, d_work, work_words,
                      stream_);
}

extern "C" int dvda_mlp_hip_pcm_crc32(dvda_mlp_hip_ctx *c, const int32_t *d_pcm, const uint64_t *d_out_off,
                                      const uint64_t *d_out_stride, unsigned bits, uint32_t *host_crc,
                                      uint64_t *host_nbytes, uint32_t n, void *stream_)
{
    if (!c || !d_pcm || !d_out_off || !d_out_stride || !host_crc || !host_nbytes)
        return DVDA_HIP_EINVAL;
    CrcReport r{};
    const int rc = report_of_decode(c, d_pcm, d_out_off, d_out_stride, bits, &n, stream_, &r);
    if (rc || n == 0)
        return rc;
    return report_down(stream_, host_crc, r.d_crc, (size_t)n * sizeof(uint32_t), host_nbytes, r.d_nbytes,
                       (size_t)n * sizeof(uint64_t));
}

extern "C" uint32_t dvda_pcm_hip_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b)
{
    // x has order 2^32 - 1 in the field, and 8 * len_b must not wrap: reduce the exponent first
    const uint64_t e = ((len_b % 0xFFFFFFFFull) * 8u) % 0xFFFFFFFFull;
    return crc::gfmul(crc_a, crc::xpow(e)) ^ crc_b;
}

// ---- the level report
extern "C" size_t dvda_pcm_hip_levels_workspace_words(uint32_t n, uint64_t max_total_frames)
{
    return report_workspace_words(LvlReport{}, n, max_total_frames);
}

extern "C" int dvda_pcm_hip_levels(const int32_t *d_pcm, uint32_t layout, unsigned bits, const dvda_pcm_crc_desc *d_desc,
                                   uint32_t n, uint64_t max_total_frames, dvda_pcm_levels *d_levels, uint32_t *d_work,
                                   size_t work_words, void *stream_)
{
    return report_run(LvlReport{d_levels}, d_pcm, layout, bits, d_desc, n, max_total_frames, d_work, work_words, stream_);
}

extern "C" int dvda_mlp_hip_pcm_levels(dvda_mlp_hip_ctx *c, const int32_t *d_pcm, const uint64_t *d_out_off,
                                       const uint64_t *d_out_stride, unsigned bits, dvda_pcm_levels *host_levels, uint32_t n,
                                       void *stream_)
{
    if (!c || !d_pcm || !d_out_off || !d_out_stride || !host_levels || !LvlReport::takes(c->set.pcm_layout, bits))
        return DVDA_HIP_EINVAL;
    LvlReport r{};
    const int rc = report_of_decode(c, d_pcm, d_out_off, d_out_stride, bits, &n, stream_, &r);
    if (rc || n == 0)
        return rc;
    return report_down(stream_, host_levels, r.d_levels, (size_t)n * sizeof(dvda_pcm_levels));
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

// ---- the compare
extern "C" size_t dvda_pcm_hip_compare_workspace_words(uint32_t n, uint64_t max_total_frames)
{
    return report_workspace_words(CmpReport{}, n, max_total_frames);
}

extern "C" int dvda_pcm_hip_compare(const int32_t *d_a, uint32_t layout_a, const dvda_pcm_crc_desc *d_desc_a,
                                    const int32_t *d_b, uint32_t layout_b, const dvda_pcm_crc_desc *d_desc_b, uint32_t n,
                                    unsigned bits, uint64_t max_total_frames, dvda_pcm_diff *d_diff, uint32_t *d_work,
                                    size_t work_words, void *stream_)
{
    return report_run(CmpReport{d_diff, d_b, layout_b, d_desc_b}, d_a, layout_a, bits, d_desc_a, n, max_total_frames, d_work,
                      work_words, stream_);
}

extern "C" int dvda_mlp_hip_pcm_compare(dvda_mlp_hip_ctx *c, const int32_t *d_pcm, const uint64_t *d_out_off,
                                        const uint64_t *d_out_stride, const int32_t *d_other, uint32_t other_layout,
                                        const dvda_pcm_crc_desc *d_other_desc, unsigned bits, dvda_pcm_diff *host_diff,
                                        uint32_t n, void *stream_)
{
    CmpReport r{nullptr, d_other, other_layout, d_other_desc};
    if (!c || !d_pcm || !d_out_off || !d_out_stride || !host_diff || !d_other || !d_other_desc ||
        !int32_layout(other_layout) || !CmpReport::takes(c->set.pcm_layout, bits))
        return DVDA_HIP_EINVAL;
    const int rc = report_of_decode(c, d_pcm, d_out_off, d_out_stride, bits, &n, stream_, &r);
    if (rc || n == 0)
        return rc;
    return report_down(stream_, host_diff, r.d_diff, (size_t)n * sizeof(dvda_pcm_diff));
}

extern "C" int dvda_pcm_hip_diff_combine(const dvda_pcm_diff *a_, const dvda_pcm_diff *b_, dvda_pcm_diff *out)
{
    if (!a_ || !b_ || !out)
        return DVDA_HIP_EINVAL;
    const dvda_pcm_diff a = *a_, b = *b_;           // (either may be `out`)
    if ((a.flags | b.flags) & DVDA_CMP_SHAPE)
        return DVDA_HIP_EINVAL;
    const bool a_none = !a.frames_a && !a.frames_b && !a.flags, b_none = !b.frames_a && !b.frames_b && !b.flags;
    if (a_none || b_none) {                         // neutral: its channel count does not reach the result
        *out = a_none ? b : a;
        return DVDA_HIP_OK;
    }
    if (a.frames_a != a.frames_b || a.channels != b.channels)
        return DVDA_HIP_EINVAL;
    dvda_pcm_diff r;
    r.frames_a = a.frames_a + b.frames_a;
    r.frames_b = a.frames_b + b.frames_b;
    r.compared = a.compared + b.compared;
    r.diff_frames = a.diff_frames + b.diff_frames;
    r.first_diff = a.first_diff < a.compared ? a.first_diff : a.compared + b.first_diff;
    r.diff_end = b.diff_end ? a.compared + b.diff_end : a.diff_end;
    const bool seam = a.diff_end == a.compared && a.compared && b.compared && b.first_diff == 0;
    r.runs = a.runs + b.runs - (seam ? 1 : 0);
    for (int c = 0; c < 8; c++) {
        r.diff_values[c] = a.diff_values[c] + b.diff_values[c];
        r.max_abs[c] = a.max_abs[c] > b.max_abs[c] ? a.max_abs[c] : b.max_abs[c];
    }
    r.channels = a.channels;
    r.flags = a.flags | b.flags;
    *out = r;
    return DVDA_HIP_OK;
}

// ---- the energy report
extern "C" size_t dvda_pcm_hip_energy_workspace_words(uint32_t n, uint64_t max_total_frames, uint32_t block_frames)
{
    if (!NrgReport::block_ok(block_frames))
        return 0;
    return report_workspace_words(NrgReport{block_frames}, n, max_total_frames);
}

extern "C" int dvda_pcm_hip_energy(const int32_t *d_pcm, uint32_t layout, const dvda_pcm_crc_desc *d_desc, uint32_t n,
                                   uint32_t block_frames, const uint32_t *d_lead, uint64_t max_total_frames,
                                   dvda_pcm_energy_block *d_blocks, const uint64_t *d_block_off, const uint64_t *d_block_cap,
                                   uint64_t *d_nblocks, uint32_t *d_work, size_t work_words, void *stream_)
{
    return report_run(NrgReport{block_frames, d_lead, d_blocks, d_block_off, d_block_cap, d_nblocks}, d_pcm, layout, 0, d_desc,
                      n, max_total_frames, d_work, work_words, stream_);
}

extern "C" int dvda_mlp_hip_pcm_energy(dvda_mlp_hip_ctx *c, const int32_t *d_pcm, const uint64_t *d_out_off,
                                       const uint64_t *d_out_stride, uint32_t block_frames,
                                       dvda_pcm_energy_block *host_blocks, uint64_t cap_blocks, uint64_t *host_first, uint32_t n,
                                       void *stream_)
{
    if (!c || !d_pcm || !d_out_off || !d_out_stride || !host_first || (!host_blocks && cap_blocks) ||
        !NrgReport::block_ok(block_frames) || !NrgReport::takes(c->set.pcm_layout, 0))
        return DVDA_HIP_EINVAL;
    NrgReport r{block_frames, nullptr, nullptr, nullptr, nullptr, nullptr, cap_blocks, host_first};
    const int rc = report_of_decode(c, d_pcm, d_out_off, d_out_stride, 0, &n, stream_, &r);
    if (rc || n == 0)
        return rc;
    return report_down(stream_, host_blocks, r.d_blocks, (size_t)host_first[n] * sizeof(dvda_pcm_energy_block));
}

static inline void nrg_add(dvda_pcm_energy_block *t, const dvda_pcm_energy_block &p)
{
    for (int c = 0; c < 8; c++) {
        t->sq_lo[c] += p.sq_lo[c];
        t->sq_hi[c] += p.sq_hi[c] + (t->sq_lo[c] < p.sq_lo[c] ? 1u : 0u);
        t->peak[c] = p.peak[c] > t->peak[c] ? p.peak[c] : t->peak[c];
    }
}

extern "C" int dvda_pcm_hip_energy_append(dvda_pcm_energy_block *track, uint64_t *n_track, uint64_t cap,
                                          const dvda_pcm_energy_block *piece, uint64_t n_piece, uint32_t block_frames)
{
    if (!n_track || (!track && cap) || (!piece && n_piece) || !NrgReport::block_ok(block_frames) || *n_track > cap)
        return DVDA_HIP_EINVAL;
    if (n_piece == 0)
        return DVDA_HIP_OK;
    const uint64_t have = *n_track;
    const bool merge = have && track[have - 1].frames < block_frames;
    // on the grid: the block the piece opens or completes has at most B frames, and exactly B when more blocks follow
    // it; behind it only the piece's last block is short
    const uint64_t head = (merge ? track[have - 1].frames : 0u) + (uint64_t)piece[0].frames;
    if (head > block_frames || (n_piece > 1 && head != block_frames))
        return DVDA_HIP_EINVAL;
    for (uint64_t j = 1; j < n_piece; j++)
        if (piece[j].frames > block_frames || (j + 1 < n_piece && piece[j].frames != block_frames))
            return DVDA_HIP_EINVAL;
    const uint64_t need = have + n_piece - (merge ? 1 : 0);
    if (need > cap)
        return DVDA_HIP_ECAPACITY;
    uint64_t j = 0;
    if (merge) {
        nrg_add(&track[have - 1], piece[0]);
        track[have - 1].frames += piece[0].frames;
        j = 1;
    }
    for (uint64_t at = have; j < n_piece; j++, at++)
        track[at] = piece[j];
    *n_track = need;
    return DVDA_HIP_OK;
}

extern "C" void dvda_pcm_hip_energy_total(const dvda_pcm_energy_block *blocks, uint64_t n, dvda_pcm_energy_block *out)
{
    dvda_pcm_energy_block r = {};
    uint64_t frames = 0;
    for (uint64_t j = 0; j < n; j++) {
        nrg_add(&r, blocks[j]);
        frames += blocks[j].frames;
        if (frames > 0xFFFFFFFFull)
            frames = 0xFFFFFFFFull;
    }
    r.frames = (uint32_t)frames;
    *out = r;
}

// ---- the word-length reduction
extern "C" size_t dvda_pcm_hip_requantize_workspace_words(uint32_t n, uint64_t max_total_frames)
{
    return report_workspace_words(RqReport{}, n, max_total_frames);
}

extern "C" int dvda_pcm_hip_requantize(const int32_t *d_in, uint32_t layout_in, const dvda_pcm_crc_desc *d_desc_in,
                                       int32_t *d_out, uint32_t layout_out, const dvda_pcm_crc_desc *d_desc_out,
                                       const uint64_t *d_frame0, uint32_t n, const dvda_pcm_requant *params,
                                       uint64_t max_total_frames, dvda_pcm_requant_report *d_report, uint32_t *d_work,
                                       size_t work_words, void *stream_)
{
    return report_run(RqReport{d_report, d_out, layout_out, d_desc_out, d_frame0, params}, d_in, layout_in, 0, d_desc_in, n,
                      max_total_frames, d_work, work_words, stream_);
}

extern "C" int dvda_mlp_hip_pcm_requantize(dvda_mlp_hip_ctx *c, int32_t *d_pcm, const uint64_t *d_out_off,
                                           const uint64_t *d_out_stride, const dvda_pcm_requant *params,
                                           const uint64_t *host_frame0, dvda_pcm_requant_report *host_report, uint32_t n,
                                           void *stream_)
{
    if (!c || !d_pcm || !d_out_off || !d_out_stride || !params || !host_report || !rq::params_ok(*params) ||
        !RqReport::takes(c->set.pcm_layout, 0))
        return DVDA_HIP_EINVAL;
    RqReport r{nullptr, d_pcm, c->set.pcm_layout, nullptr, nullptr, params, host_frame0};
    const int rc = report_of_decode(c, d_pcm, d_out_off, d_out_stride, 0, &n, stream_, &r);
    if (rc || n == 0)
        return rc;
    return report_down(stream_, host_report, r.d_report, (size_t)n * sizeof(dvda_pcm_requant_report));
}

extern "C" int32_t dvda_pcm_hip_requant_value(int32_t v, uint64_t frame, uint32_t channel, const dvda_pcm_requant *params,
                                              int *clipped)
{
    return value_or_bad(params && rq::params_ok(*params), clipped, [&](uint32_t *cl) {
        const rq::Par p = rq::par_of(*params);
        const uint64_t z = p.mode == DVDA_RQ_TPDF && p.s ? rq::noise_word(p.seed, frame >> 2, channel) : 0;
        return rq::value(v, p, rq::noise_field(z, (uint32_t)frame & 3u), cl);
    });
}

// ---- the decimation
extern "C" size_t dvda_pcm_hip_decimate_workspace_words(uint32_t n, uint64_t max_total_out_frames)
{
    return report_workspace_words(DcReport{}, n, max_total_out_frames);
}

extern "C" int dvda_pcm_hip_decimate(const int32_t *d_in, uint32_t layout_in, const dvda_pcm_crc_desc *d_desc_in,
                                     int32_t *d_out, uint32_t layout_out, const dvda_pcm_crc_desc *d_desc_out,
                                     const dvda_pcm_decim_piece *d_piece, uint32_t n, uint32_t ratio, unsigned bits,
                                     uint64_t max_total_out_frames, dvda_pcm_decim_report *d_report, uint32_t *d_work,
                                     size_t work_words, void *stream_)
{
    return report_run(DcReport{{d_report, d_out, layout_out, d_desc_out}, d_piece, ratio}, d_in, layout_in, bits, d_desc_in, n,
                      max_total_out_frames, d_work, work_words, stream_);
}

extern "C" int dvda_mlp_hip_pcm_decimate(dvda_mlp_hip_ctx *c, const int32_t *d_pcm, const uint64_t *d_out_off,
                                         const uint64_t *d_out_stride, uint32_t ratio, unsigned bits, int32_t *d_dst,
                                         uint32_t layout_dst, const uint64_t *host_dst_off, const uint64_t *host_dst_stride,
                                         dvda_pcm_decim_report *host_report, uint32_t n, void *stream_)
{
    if (!c || !d_pcm || !d_out_off || !d_out_stride || !d_dst || !host_dst_off || !host_dst_stride || !host_report ||
        !dcm::ratio_ok(ratio) || !int32_layout(layout_dst) || !DcReport::takes(c->set.pcm_layout, bits))
        return DVDA_HIP_EINVAL;
    DcReport r{{nullptr, d_dst, layout_dst, nullptr, host_dst_off, host_dst_stride}, nullptr, ratio};
    const int rc = report_of_decode(c, d_pcm, d_out_off, d_out_stride, bits, &n, stream_, &r);
    if (rc || n == 0)
        return rc;
    return report_down(stream_, host_report, r.d_report, (size_t)n * sizeof(dvda_pcm_decim_report));
}

extern "C" const int32_t *dvda_pcm_hip_decim_taps(uint32_t ratio, uint32_t *n)
{
    if (n)
        *n = dcm::ratio_ok(ratio) ? dcm::taps_of(ratio) : 0u;
    return ratio == 2 ? dcm::Taps<2>::h : ratio == 4 ? dcm::Taps<4>::h : nullptr;
}

extern "C" uint64_t dvda_pcm_hip_decim_out_frames(uint64_t frame0, uint64_t own, uint32_t ratio)
{
    return dcm::out_frames(frame0, own, ratio);
}

extern "C" int32_t dvda_pcm_hip_decim_value(const int32_t *window, uint32_t ratio, unsigned bits, int *clipped)
{
    return value_or_bad(window && dcm::ratio_ok(ratio) && dcm::depth_ok(bits), clipped, [&](uint32_t *cl) {
        return ratio == 2 ? dcm::value<2>(window, bits, cl) : dcm::value<4>(window, bits, cl);
    });
}

// ---- the resampler
extern "C" size_t dvda_pcm_hip_resample_workspace_words(uint32_t n, uint64_t max_total_out_frames)
{
    return report_workspace_words(RsReport{}, n, max_total_out_frames);
}

extern "C" int dvda_pcm_hip_resample(const int32_t *d_in, uint32_t layout_in, const dvda_pcm_crc_desc *d_desc_in,
                                     int32_t *d_out, uint32_t layout_out, const dvda_pcm_crc_desc *d_desc_out,
                                     const dvda_pcm_decim_piece *d_piece, uint32_t n, unsigned bits,
                                     uint64_t max_total_out_frames, dvda_pcm_decim_report *d_report, uint32_t *d_work,
                                     size_t work_words, void *stream_)
{
    return report_run(RsReport{{d_report, d_out, layout_out, d_desc_out}, d_piece}, d_in, layout_in, bits, d_desc_in, n,
                      max_total_out_frames, d_work, work_words, stream_);
}

extern "C" int dvda_mlp_hip_pcm_resample(dvda_mlp_hip_ctx *c, const int32_t *d_pcm, const uint64_t *d_out_off,
                                         const uint64_t *d_out_stride, unsigned bits, int32_t *d_dst, uint32_t layout_dst,
                                         const uint64_t *host_dst_off, const uint64_t *host_dst_stride,
                                         dvda_pcm_decim_report *host_report, uint32_t n, void *stream_)
{
    if (!c || !d_pcm || !d_out_off || !d_out_stride || !d_dst || !host_dst_off || !host_dst_stride || !host_report ||
        !int32_layout(layout_dst) || !RsReport::takes(c->set.pcm_layout, bits))
        return DVDA_HIP_EINVAL;
    RsReport r{{nullptr, d_dst, layout_dst, nullptr, host_dst_off, host_dst_stride}};
    const int rc = report_of_decode(c, d_pcm, d_out_off, d_out_stride, bits, &n, stream_, &r);
    if (rc || n == 0)
        return rc;
    return report_down(stream_, host_report, r.d_report, (size_t)n * sizeof(dvda_pcm_decim_report));
}

extern "C" const int32_t *dvda_pcm_hip_resample_taps(uint32_t *phases, uint32_t *taps)
{
    if (phases)
        *phases = rsm::PHASES;
    if (taps)
        *taps = rsm::TAPS;
    return &rsm::Table::g[0][0];
}

extern "C" uint64_t dvda_pcm_hip_resample_out_frames(uint64_t frame0, uint64_t own) { return rsm::out_frames(frame0, own); }

extern "C" int32_t dvda_pcm_hip_resample_value(const int32_t *window, uint32_t phase, unsigned bits, int *clipped)
{
    return value_or_bad(window && phase < rsm::PHASES && rsm::depth_ok(bits), clipped,
                        [&](uint32_t *cl) { return rsm::value(window, phase, bits, cl); });
}

// ---- the channel mix
extern "C" size_t dvda_pcm_hip_mix_workspace_words(uint32_t n, uint64_t max_total_frames)
{
    return report_workspace_words(MixReport{}, n, max_total_frames);
}

extern "C" int dvda_pcm_hip_mix(const int32_t *d_in, uint32_t layout_in, const dvda_pcm_crc_desc *d_desc_in, int32_t *d_out,
                                uint32_t layout_out, const dvda_pcm_crc_desc *d_desc_out, const dvda_pcm_mix *d_mix,
                                uint32_t n, unsigned bits, uint64_t max_total_frames, dvda_pcm_mix_report *d_report,
                                uint32_t *d_work, size_t work_words, void *stream_)
{
    return report_run(MixReport{{d_report, d_out, layout_out, d_desc_out}, d_mix}, d_in, layout_in, bits, d_desc_in, n,
                      max_total_frames, d_work, work_words, stream_);
}

extern "C" int dvda_mlp_hip_pcm_mix(dvda_mlp_hip_ctx *c, const int32_t *d_pcm, const uint64_t *d_out_off,
                                    const uint64_t *d_out_stride, int32_t *d_out, const uint64_t *d_mix_off,
                                    const uint64_t *d_mix_stride, const dvda_pcm_mix *host_mix, unsigned bits,
                                    dvda_pcm_mix_report *host_report, uint32_t n, void *stream_)
{
    if (!c || !d_pcm || !d_out_off || !d_out_stride || !d_out || !d_mix_off || !d_mix_stride || !host_mix || !host_report ||
        !MixReport::takes(c->set.pcm_layout, bits))
        return DVDA_HIP_EINVAL;
    int rc = report_clamp(c, &n);
    if (rc || n == 0)
        return rc;
    // where the output's regions lie, on the host: the stage writes them into the output's descriptors
    std::vector<uint64_t> off(n), stride(n);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpy(off.data(), d_mix_off, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(stride.data(), d_mix_stride, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    MixReport r{{nullptr, d_out, c->set.pcm_layout, nullptr, off.data(), stride.data()}, nullptr, host_mix};
    rc = report_of_decode(c, d_pcm, d_out_off, d_out_stride, bits, &n, stream_, &r);
    if (rc || n == 0)
        return rc;
    return report_down(stream_, host_report, r.d_report, (size_t)n * sizeof(dvda_pcm_mix_report));
}

extern "C" unsigned dvda_pcm_hip_speaker_mask(unsigned assignment)
{
    // speaker bits per DVD-Audio channel assignment, the channels of a buffer in ascending order of their bits
    enum { FL = 0x1, FR = 0x2, FC = 0x4, LF = 0x8, BL = 0x10, BR = 0x20, BC = 0x100 };
    static const unsigned mask[21] = {
        FC, FL | FR, FL | FR | BC, FL | FR | BL | BR, FL | FR | LF, FL | FR | LF | BC, FL | FR | LF | BL | BR,
        FL | FR | FC, FL | FR | FC | BC, FL | FR | FC | BL | BR, FL | FR | FC | LF, FL | FR | FC | LF | BC,
        FL | FR | FC | LF | BL | BR, FL | FR | FC | BC, FL | FR | FC | BL | BR, FL | FR | FC | LF,
        FL | FR | FC | LF | BC, FL | FR | FC | LF | BL | BR, FL | FR | BL | BR | LF, FL | FR | BL | BR | FC,
        FL | FR | BL | BR | FC | LF};
    return assignment < 21 ? mask[assignment] : 0;
}

extern "C" int dvda_pcm_hip_mix_matrix(unsigned speaker_mask, uint32_t out_channels, uint32_t flags, dvda_pcm_mix *out)
{
    constexpr int64_t ONE = 1ll << 30, A = 759250125, HALF = 1ll << 29;
    if (!out || speaker_mask == 0 || (speaker_mask & ~0x13Fu) || (out_channels != 1 && out_channels != 2) ||
        (flags & ~(DVDA_MIX_UNITY | DVDA_MIX_LFE)))
        return DVDA_HIP_EINVAL;
    const int64_t lfe = (flags & DVDA_MIX_LFE) ? A : 0;
    // the weights of the buffer's channels, the c-th set bit of the mask being channel c
    int64_t w[2][8] = {};
    uint32_t in = 0;
    for (unsigned bit = 0; bit < 9; bit++) {
        if (!(speaker_mask >> bit & 1u))
            continue;
        int64_t l = 0, r = 0;
        switch (1u << bit) {
        case 0x1: l = ONE; break;
        case 0x2: r = ONE; break;
        case 0x4: l = r = A; break;
        case 0x8: l = r = lfe; break;
        case 0x10: l = A; break;
        case 0x20: r = A; break;
        case 0x100: l = r = HALF; break;
        }
        w[0][in] = l;
        w[1][in] = r;
        in++;
    }
    dvda_pcm_mix m = {};
    m.in_channels = in;
    m.out_channels = out_channels;
    if (out_channels == 1)
        for (uint32_t c = 0; c < in; c++)
            w[0][c] += w[1][c];
    if (flags & DVDA_MIX_UNITY) {
        for (uint32_t o = 0; o < out_channels; o++)
            for (uint32_t c = 0; c < in; c++)
                m.coef[o][c] = (int32_t)(out_channels == 1 ? w[0][c] >> 1 : w[o][c]);
    } else {
        int64_t S = 0;
        for (uint32_t o = 0; o < out_channels; o++) {
            int64_t sum = 0;
            for (uint32_t c = 0; c < in; c++)
                sum += w[o][c];
            S = sum > S ? sum : S;
        }
        // (S == 0: an LFE alone without the flag; nothing of it reaches the output)
        for (uint32_t o = 0; o < out_channels; o++)
            for (uint32_t c = 0; c < in; c++)
                m.coef[o][c] = S ? (int32_t)((w[o][c] << 30) / S) : 0;
    }
    *out = m;
    return DVDA_HIP_OK;
}

extern "C" int dvda_pcm_hip_mix_valid(const dvda_pcm_mix *m) { return m && mix::valid(*m) ? 1 : 0; }

extern "C" int32_t dvda_pcm_hip_mix_value(const int32_t *x, const dvda_pcm_mix *m, uint32_t o, unsigned bits, int *clipped)
{
    return value_or_bad(x && m && mix::valid(*m) && o < m->out_channels && mix::depth_ok(bits), clipped,
                        [&](uint32_t *cl) { return mix::value(x, *m, o, bits, cl); });
}
