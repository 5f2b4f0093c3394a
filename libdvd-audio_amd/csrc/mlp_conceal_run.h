// mlp_conceal_run.h -- conceal mode, host side (the kernels: mlp_conceal.h; the rule: include/dvda_mlp_hip.h).
// conceal_run is what dvda_mlp_hip_decode goes on with when the mode is on: it plans the damaged streams, decodes
// their kept ranges again through a second context and lays the result out in the caller's buffer.
#pragma once
#include <math.h>
#include <string.h>

#include "mlp_ctx.h"

extern "C" int dvda_mlp_hip_set_conceal(dvda_mlp_hip_ctx *c, int on)
{
    if (!c || (on && c->pp.mode != DVDA_PRESENT_FULL))
        return DVDA_HIP_EINVAL;     // (conceal mode of a presentation: not built)
    c->cc.on = on != 0;
    c->cc.spans.clear();
    c->cc.info.clear();
    c->cc.ran = false;
    return DVDA_HIP_OK;
}

extern "C" int dvda_mlp_hip_conceal_edges(dvda_mlp_hip_ctx *c, uint32_t stream, dvda_mlp_conceal_edges *out, void *stream_)
{
    if (!c || !out)
        return DVDA_HIP_EINVAL;
    if (!c->indexed || !c->cc.ran)
        return DVDA_HIP_ESTATE;
    if (stream >= c->n_streams || stream >= c->cc.h_streams.size())
        return DVDA_HIP_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream_));
    if (stream < c->cc.edges.size() && c->cc.edges[stream].reserved) {
        *out = c->cc.edges[stream];
        out->reserved = 0;
        return DVDA_HIP_OK;
    }
    // a clean stream: all of it is kept; the history is that of its last live segment (no launch: a few small copies)
    const StreamRec &r = c->cc.h_streams[stream];
    memset(out, 0, sizeof(*out));
    out->kept_end = out->kept_bytes = r.consumed;
    out->kept_frames = r.rows;
    uint64_t soff = 0, slen = 0;
    HIP_TRY(hipMemcpy(&soff, c->d_soff + stream, sizeof(soff), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&slen, c->d_slen + stream, sizeof(slen), hipMemcpyDeviceToHost));
    out->ends_kept = 1;
    if (r.first_seg == 0xFFFFFFFFu || r.consumed < 4 || r.consumed > slen)
        return DVDA_HIP_OK;
    uint8_t head[4];
    HIP_TRY(hipMemcpy(head, c->d_bytes + soff, sizeof(head), hipMemcpyDeviceToHost));
    out->t_first = ((uint32_t)head[2] << 8) | head[3];
    out->t_end = (out->t_first + (uint32_t)r.rows) & 0xFFFFu;
    uint32_t n_cand = 0;
    HIP_TRY(hipMemcpy(&n_cand, c->d_n_cand, sizeof(n_cand), hipMemcpyDeviceToHost));
    if (n_cand > c->max_segments)
        n_cand = c->max_segments;
    uint32_t last = 0xFFFFFFFFu;
    if (r.first_seg < n_cand) {
        uint32_t n = n_cand - r.first_seg;
        if (n > r.n_seg)
            n = r.n_seg;
        std::vector<SegRec> segs(n);
        if (n)
            HIP_TRY(hipMemcpy(segs.data(), c->d_seg + r.first_seg, (size_t)n * sizeof(SegRec), hipMemcpyDeviceToHost));
        for (uint32_t k = 0; k < n; k++)
            if (segs[k].stream == stream && !(segs[k].flags & SEG_DEAD))
                last = r.first_seg + k;
    }
    if (last != 0xFFFFFFFFu && dvda_mlp_hip_segment_fir(c, last, out->fir, stream_) != DVDA_HIP_OK)
        return DVDA_HIP_ENODEV;
    return DVDA_HIP_OK;
}

extern "C" int dvda_mlp_hip_conceal_spans(dvda_mlp_hip_ctx *c, uint32_t stream, dvda_mlp_conceal_span *spans,
                                          uint32_t cap, uint32_t *n, void *stream_)
{
    if (!c || !n || (cap && !spans))
        return DVDA_HIP_EINVAL;
    if (!c->indexed)
        return DVDA_HIP_ESTATE;
    if (stream >= c->n_streams)
        return DVDA_HIP_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream_));
    *n = 0;
    if (stream >= c->cc.spans.size())
        return DVDA_HIP_OK;
    const std::vector<dvda_mlp_conceal_span> &v = c->cc.spans[stream];
    *n = (uint32_t)v.size();
    for (uint32_t k = 0; k < cap && k < v.size(); k++)
        spans[k] = v[k];
    return DVDA_HIP_OK;
}

namespace {
struct CcItem {                 // a kept byte range of a damaged stream
    uint64_t a, b;              // absolute offsets in the caller's buffer
    uint32_t t_first;           // input timing at a (t_first + frames: behind its last unit)
    uint32_t cause, flags;      // the span in front of it: DVDA_ST_* bits, DVDA_CONCEAL_* flags
    uint32_t state;             // 0: to decode (fresh), 1: decoded clean
    uint32_t round, piece;      // decoded by that round as that piece
    uint64_t scr_off, cap;      // its PCM in the round's scratch (int32 units), capacity / channel stride there (frames)
    uint64_t frames, units;
    uint32_t status, stream;
    uint32_t fir_slot;          // its FIR history behind its last unit: edge_firs[fir_slot] (decoded clean)
};
struct CcStream {
    uint32_t id;
    std::vector<CcItem> items;
    uint32_t tail_cause, tail_flags;
};
} // namespace

// frames of silence for a span of B bytes whose timing says g (mod 65536): g + 65536 w, w >= 0 the integer whose bytes per
// frame come closest to m, the stream's mean over its kept ranges (no mean: g)
static uint64_t conceal_gap(uint64_t B, uint32_t g, double m)
{
    if (!(m > 0.0))
        return g;
    double w0 = floor(((double)B / m - (double)g) / 65536.0);
    if (w0 < 0.0)
        w0 = 0.0;
    uint64_t best = 0;
    double bd = 0.0;
    for (int k = 0; k < 2; k++) {
        const uint64_t G = (uint64_t)g + 65536ull * ((uint64_t)w0 + (uint64_t)k);
        const double d = G ? fabs((double)B / (double)G - m) : INFINITY;
        if (k == 0 || d < bd) {
            best = G;
            bd = d;
        }
    }
    return best;
}

// The blocking decode is through; conceal mode: the damaged streams are planned, their kept ranges decoded again in
// rounds by a second context (fresh state, each range a stream of its own), and the result laid out in the caller's
// buffer with zeros between the ranges.  A batch without damage returns after one read of the stream records.
static int conceal_run(dvda_mlp_hip_ctx *c, int32_t *d_pcm, const uint64_t *d_out_off, const uint64_t *d_out_stride,
                       hipStream_t st)
{
    const uint32_t ns = c->n_streams;
    c->cc.spans.assign(ns, std::vector<dvda_mlp_conceal_span>());
    c->cc.info.assign(ns, ConcealInfo());
    c->cc.edges.clear();
    c->cc.ran = false;
    std::vector<StreamRec> h(ns);
    HIP_TRY(hipMemcpyAsync(h.data(), c->d_streams, (size_t)ns * sizeof(StreamRec), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    c->cc.h_streams = h;
    c->cc.ran = true;
    std::vector<uint32_t> dam;
    for (uint32_t i = 0; i < ns; i++)
        if (h[i].status & CONCEAL_DAMAGE)
            dam.push_back(i);
    if (dam.empty())
        return DVDA_HIP_OK;
    c->cc.ran = false;                          // (until the batch is composed: a failure below leaves no edges)
    {
        dvda_mlp_conceal_edges none;
        memset(&none, 0, sizeof(none));
        c->cc.edges.assign(ns, none);
    }
    std::vector<int32_t> edge_firs;             // [slot][2][48]: the history behind every range that decoded clean
    std::vector<uint64_t> soff(ns), slen(ns), oo(ns), os(ns);
    HIP_TRY(hipMemcpyAsync(soff.data(), c->d_soff, (size_t)ns * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(slen.data(), c->d_slen, (size_t)ns * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(oo.data(), d_out_off, (size_t)ns * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(os.data(), d_out_stride, (size_t)ns * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));

    int rc;
    std::vector<ConcealPlan> plans;
    auto run_plan = [&](dvda_mlp_hip_ctx *x, uint32_t n) -> int {
        int r = c->cc.d_plan.grow(n);
        if (r)
            return r;
        hipLaunchKernelGGL(k_conceal_plan, dim3((n + 63) / 64), dim3(64), 0, st, x->d_bytes, x->d_soff, x->d_slen, x->d_seg,
                           x->d_seg_status, x->d_n_cand, x->max_segments, x->d_streams, n, c->cc.d_plan);
        HIP_TRY(hipGetLastError());
        plans.resize(n);
        HIP_TRY(hipMemcpyAsync(plans.data(), c->cc.d_plan, (size_t)n * sizeof(ConcealPlan), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return DVDA_HIP_OK;
    };
    // a plan's ranges (relative to `base`, the piece `len` bytes long) -> items; `in` = the span in front of the piece
    auto items_of = [](const ConcealPlan &P, uint64_t base, uint32_t cause_in, uint32_t flags_in, std::vector<CcItem> &out,
                       uint32_t &tail) {
        const uint32_t n = P.n <= CONCEAL_MAX_RANGES ? P.n : 0u;       // (0xFFFFFFFF: not planned -- nothing kept)
        for (uint32_t k = 0; k < n; k++) {
            CcItem it;
            memset(&it, 0, sizeof(it));
            it.a = base + P.r[k].a;
            it.b = base + P.r[k].b;
            it.t_first = P.r[k].t_first;
            it.cause = P.r[k].cause | (k == 0 ? cause_in : 0u);
            it.flags = k == 0 ? flags_in : 0u;
            out.push_back(it);
        }
        tail = (P.n <= CONCEAL_MAX_RANGES ? P.tail_cause : DVDA_ST_ENVELOPE) | (n == 0 ? cause_in : 0u);
    };

    // ---- round 0: the caller's index
    if ((rc = run_plan(c, ns)) != 0)
        return rc;
    std::vector<CcStream> S;
    for (uint32_t i : dam) {
        CcStream cs;
        cs.id = i;
        cs.tail_flags = 0;
        items_of(plans[i], soff[i], 0u, 0u, cs.items, cs.tail_cause);
        S.push_back(cs);
    }
    const uint32_t layout = c->set.pcm_layout;
    const uint64_t vb = layout == DVDA_PCM_WAV24 ? 3 : layout == DVDA_PCM_WAV16 ? 2 : 4;
    auto chans = [&](uint32_t i) { return (uint64_t)channel_count((h[i].sync >> 16) & 0x1Fu); };

    // ---- rounds 1 .. CONCEAL_ROUNDS - 1: every range not yet decoded clean, fresh
    for (uint32_t round = 1; round < CONCEAL_ROUNDS; round++) {
        uint32_t np = 0;
        for (CcStream &cs : S)
            for (CcItem &it : cs.items)
                if (it.state == 0) {
                    it.stream = cs.id;
                    it.piece = np++;
                }
        if (np == 0)
            break;
        // gather table [3 np], then the second index's ranges and outputs [4 np]
        std::vector<uint64_t> up(7 * (size_t)np);
        std::vector<CcItem *> pc(np);
        uint64_t pos = 0;
        for (CcStream &cs : S) {
            for (CcItem &it : cs.items) {
                if (it.state != 0)
                    continue;
                const uint32_t q = it.piece;
                const uint64_t len = it.b - it.a;
                pc[q] = &it;
                up[3 * (size_t)q] = it.a;
                up[3 * (size_t)q + 1] = pos;
                up[3 * (size_t)q + 2] = len;
                up[3 * (size_t)np + q] = pos;
                up[4 * (size_t)np + q] = len;
                pos += (len + 15) & ~(uint64_t)15;
            }
        }
        if ((rc = c->cc.d_bytes.grow(pos + 64)) != 0 ||
            (rc = c->cc.d_tab.grow(7 * (uint64_t)np)) != 0 ||
            (rc = c->cc.d_fir.grow(2 * 48 * (uint64_t)np)) != 0)
            return rc;
        HIP_TRY(hipMemcpyAsync(c->cc.d_tab, up.data(), up.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(c->cc.d_bytes, 0, pos + 64, st));
        hipLaunchKernelGGL(k_conceal_gather, dim3(16, np < 65535u ? np : 65535u), dim3(256), 0, st, c->d_bytes, c->cc.d_bytes,
                           c->cc.d_tab, np);
        HIP_TRY(hipGetLastError());
        // FIR history of the ranges' decoders: a range that starts at its stream's first byte starts with what the caller's
        // decode started that stream with (dvda_mlp_hip_set_initial_fir: its kept PCM is then exactly the output without
        // conceal mode); every other range with zeros, given explicitly -- a range that starts at a major sync whose first
        // block continues the history (DVDA_ST_CHAINED) is decoded with zero history there, as the oracle decodes it, not
        // refused
        HIP_TRY(hipMemsetAsync(c->cc.d_fir, 0, 2 * 48 * (size_t)np * sizeof(int32_t), st));
        if (c->set.d_init_fir)
            for (uint32_t q = 0; q < np; q++)
                if (pc[q]->a == soff[pc[q]->stream])
                    HIP_TRY(hipMemcpyAsync(c->cc.d_fir + 2 * 48 * (size_t)q, c->set.d_init_fir + 2 * 48 * (size_t)pc[q]->stream,
                                           2 * 48 * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        // the second context: as large as the caller's in segments (the ranges hold a part of its candidates)
        if (!c->cc.child || c->cc.child->max_streams < np) {
            dvda_mlp_hip_destroy(c->cc.child);
            c->cc.child = nullptr;
            HIP_TRY(hipStreamSynchronize(st));
            if ((rc = dvda_mlp_hip_create(&c->cc.child, c->device, np < 64 ? 64 : np, c->max_segments)) != 0)
                return rc;
            c->cc.child->idx_graph_state = -1;
        }
        dvda_mlp_hip_ctx *x = c->cc.child;
        x->set = c->set;
        x->set.d_init_fir = c->cc.d_fir;        // (its streams are the ranges: their histories, not the caller's)
        x->cc.on = false;
        const uint64_t *d_x = c->cc.d_tab + 3 * (size_t)np;
        if ((rc = dvda_mlp_hip_index(x, c->cc.d_bytes, pos, d_x, d_x + np, np, st)) != 0)
            return rc;
        std::vector<StreamRec> xh(np);
        HIP_TRY(hipMemcpyAsync(xh.data(), x->d_streams, (size_t)np * sizeof(StreamRec), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        // each range's scratch holds what its access units decode to at the standard timing (not the stream's capacity:
        // the memory follows the damage); a range that needs more (DVDA_ST_OVERFLOW, non-standard timing) is decoded
        // once more with the size it reported, up to its stream's capacity
        for (uint32_t q = 0; q < np; q++) {
            const uint64_t std_rows = xh[q].frames * rows_per_au((xh[q].sync >> 8) & 0xFu);
            pc[q]->cap = std_rows < os[pc[q]->stream] ? std_rows : os[pc[q]->stream];
        }
        for (int attempt = 0; attempt < 2; attempt++) {
            uint64_t scr = 0;
            for (uint32_t q = 0; q < np; q++) {
                const uint64_t C = chans(pc[q]->stream), cap = pc[q]->cap;
                pc[q]->scr_off = scr;
                up[5 * (size_t)np + q] = scr;
                up[6 * (size_t)np + q] = cap;
                scr += vb == 4 ? C * cap : (cap * C * vb + 3) / 4 + 4;
            }
            if ((rc = c->cc.d_scr[round].grow(scr + 16)) != 0)
                return rc;
            HIP_TRY(hipMemcpyAsync(c->cc.d_tab + 5 * (size_t)np, up.data() + 5 * (size_t)np, 2 * (size_t)np * sizeof(uint64_t),
                                   hipMemcpyHostToDevice, st));
            if ((rc = dvda_mlp_hip_decode(x, c->cc.d_scr[round], d_x + 2 * (size_t)np, d_x + 3 * (size_t)np, st)) != 0)
                return rc;
            HIP_TRY(hipMemcpyAsync(xh.data(), x->d_streams, (size_t)np * sizeof(StreamRec), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            bool redo = false;
            for (uint32_t q = 0; q < np; q++)
                if ((xh[q].status & DVDA_ST_OVERFLOW) && xh[q].rows > pc[q]->cap && pc[q]->cap < os[pc[q]->stream]) {
                    pc[q]->cap = xh[q].rows < os[pc[q]->stream] ? xh[q].rows : os[pc[q]->stream];
                    redo = true;
                }
            if (!redo)
                break;
        }
        // the history behind every range of this round, while the child's index is this round's (it is indexed again in
        // the next one): dvda_mlp_hip_conceal_edges hands out the last kept range's
        if ((rc = c->cc.d_edge_fir.grow(96 * (uint64_t)np)) != 0)
            return rc;
        hipLaunchKernelGGL(k_conceal_edge_fir, dim3(np), dim3(128), 0, st, x->d_seg, x->d_n_cand, x->max_segments, x->d_streams,
                           np, x->d_fir, x->iir_lanes, c->cc.d_edge_fir);
        HIP_TRY(hipGetLastError());
        std::vector<int32_t> round_firs(96 * (size_t)np);
        HIP_TRY(hipMemcpyAsync(round_firs.data(), c->cc.d_edge_fir, round_firs.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const bool last = round + 1 == CONCEAL_ROUNDS;
        bool again = false;
        // (a range whose decode reports DVDA_ST_ENVELOPE is not trusted either: the caller's streams may carry it, a range
        //  decoded again must come out inside the envelope)
        for (uint32_t q = 0; q < np; q++)
            again |= (xh[q].status & (CONCEAL_DAMAGE | DVDA_ST_ENVELOPE)) != 0;
        if (again && !last && (rc = run_plan(x, np)) != 0)
            return rc;
        for (CcStream &cs : S) {
            std::vector<CcItem> nv;
            uint32_t carry = 0, carry_flags = 0;        // a span behind a range: in front of the next one
            for (CcItem &it : cs.items) {
                it.cause |= carry;
                it.flags |= carry_flags;
                carry = carry_flags = 0;
                if (it.state != 0) {
                    nv.push_back(it);
                    continue;
                }
                const StreamRec &r = xh[it.piece];
                if (!(r.status & (CONCEAL_DAMAGE | DVDA_ST_ENVELOPE))) {
                    it.state = 1;
                    it.round = round;
                    it.frames = r.rows;
                    it.units = r.frames;
                    it.status = r.status;
                    it.fir_slot = (uint32_t)(edge_firs.size() / 96);
                    edge_firs.insert(edge_firs.end(), round_firs.begin() + 96 * (size_t)it.piece,
                                     round_firs.begin() + 96 * (size_t)it.piece + 96);
                    nv.push_back(it);
                } else if (last) {
                    // still damaged after the last round: concealed whole
                    carry = it.cause | (r.status & (CONCEAL_DAMAGE | DVDA_ST_ENVELOPE));
                    carry_flags = it.flags | DVDA_CONCEAL_ROUNDS;
                } else {
                    items_of(plans[it.piece], it.a, it.cause, it.flags, nv, carry);
                }
            }
            cs.tail_cause |= carry;
            cs.tail_flags |= carry_flags;
            cs.items.swap(nv);
        }
    }

    // ---- layout: kept ranges in order, silence between them
    std::vector<ConcealOp> moves, fills;
    for (CcStream &cs : S) {
        const uint32_t i = cs.id;
        const uint64_t C = chans(i);
        uint64_t K = 0, F = 0, units = 0;
        uint32_t benign = 0;
        bool ovf = false;                       // a range whose own decode did not fit
        for (const CcItem &it : cs.items) {
            ovf |= (it.status & DVDA_ST_OVERFLOW) != 0;
            K += it.b - it.a;
            F += it.frames;
            units += it.units;
            benign |= it.status & DVDA_ST_BENIGN;
        }
        const double m = K && F ? (double)K / (double)F : 0.0;
        std::vector<dvda_mlp_conceal_span> sp;
        std::vector<ConcealOp> mv, fl;
        uint64_t pos = 0;
        const CcItem *prev = nullptr;
        for (const CcItem &it : cs.items) {
            dvda_mlp_conceal_span s;
            memset(&s, 0, sizeof(s));
            s.cause = it.cause;
            s.flags = it.flags;
            s.byte_end = it.a - soff[i];
            if (!prev) {
                if (it.a > soff[i]) {
                    s.flags |= DVDA_CONCEAL_LEADING;
                    sp.push_back(s);
                }
            } else {
                const uint32_t g = (it.t_first - (uint32_t)(prev->t_first + prev->frames)) & 0xFFFFu;
                const uint64_t G = conceal_gap(it.a - prev->b, g, m);
                s.first_frame = pos;
                s.frames = G;
                s.byte_off = prev->b - soff[i];
                sp.push_back(s);
                if (G) {
                    ConcealOp o = {oo[i], 0, pos, G, os[i], 0, (uint32_t)C, 0};
                    fl.push_back(o);
                }
                pos += G;
            }
            if (it.frames) {
                ConcealOp o = {oo[i], it.scr_off, pos, it.frames, os[i], it.cap, (uint32_t)C, it.round};
                mv.push_back(o);
            }
            pos += it.frames;
            prev = &it;
        }
        const uint64_t end = soff[i] + slen[i];
        if (!prev || prev->b < end) {
            dvda_mlp_conceal_span s;
            memset(&s, 0, sizeof(s));
            s.first_frame = pos;
            s.byte_off = prev ? prev->b - soff[i] : 0;
            s.byte_end = slen[i];
            s.cause = cs.tail_cause;
            s.flags = cs.tail_flags | DVDA_CONCEAL_TRAILING | (prev ? 0u : DVDA_CONCEAL_LEADING);
            sp.push_back(s);
        }
        uint32_t status = DVDA_ST_CONCEALED | benign;
        if (pos > os[i] || ovf)
            status |= DVDA_ST_OVERFLOW;         // pcm_frames = the capacity needed; the region holds no concealed output
        else {
            moves.insert(moves.end(), mv.begin(), mv.end());
            fills.insert(fills.end(), fl.begin(), fl.end());
        }
        // (the composed record is the host's: the index's own record stays as the decode left it, so that a second decode of
        //  the same index -- after DVDA_ST_OVERFLOW -- starts from what the index found, conceal mode on or off)
        c->cc.info[i].valid = 1;
        c->cc.info[i].status = status;
        c->cc.info[i].rows = pos;
        c->cc.info[i].frames = units;
        c->cc.spans[i].swap(sp);
        dvda_mlp_conceal_edges &e = c->cc.edges[i];
        e.reserved = 1;                         // (valid; handed out as 0)
        e.kept_bytes = K;
        e.kept_frames = F;
        if (prev) {
            const CcItem &first = cs.items.front();
            e.kept_begin = first.a - soff[i];
            e.kept_end = prev->b - soff[i];
            e.t_first = first.t_first;
            e.t_end = (uint32_t)(prev->t_first + prev->frames) & 0xFFFFu;
            e.ends_kept = prev->b >= end;
            memcpy(e.fir, edge_firs.data() + 96 * (size_t)prev->fir_slot, sizeof(e.fir));
        }
    }
    c->cc.ran = true;
    const uint32_t nm = (uint32_t)moves.size(), nf = (uint32_t)fills.size();
    if (nm + nf) {
        if ((rc = c->cc.d_ops.grow((uint64_t)nm + nf)) != 0)
            return rc;
        std::vector<ConcealOp> ops(moves);
        ops.insert(ops.end(), fills.begin(), fills.end());
        HIP_TRY(hipMemcpyAsync(c->cc.d_ops, ops.data(), ops.size() * sizeof(ConcealOp), hipMemcpyHostToDevice, st));
        ConcealSrc srcs;
        memset(&srcs, 0, sizeof(srcs));
        for (uint32_t r = 0; r < CONCEAL_ROUNDS; r++)
            srcs.p[r] = c->cc.d_scr[r];
        if (nm)
            hipLaunchKernelGGL(k_conceal_move, dim3(64, nm < 65535u ? nm : 65535u), dim3(256), 0, st, c->cc.d_ops, nm,
                               layout, d_pcm, srcs);
        if (nf)
            hipLaunchKernelGGL(k_conceal_fill, dim3(64, nf < 65535u ? nf : 65535u), dim3(256), 0, st, c->cc.d_ops + nm, nf,
                               layout, d_pcm);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
    }
    return DVDA_HIP_OK;
}
