// klt_api.hip -- C ABI of the KLT front-end (include/xrslam_hip.h, plug point #1).
// Host side of xrslam::Image for gfx950: buffer management, launches on the
// context's stream, and the order-defining selections (host_select.hpp).
#include "../../include/xrslam_hip.h"
#include "common.hip.h"
#include "group.hip.h"
#include "host/pixel_format.hpp"
#include "host_select.hpp"
#include "klt_kernels.hip.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <optional>
#include <string>
#if defined(__x86_64__)
#include <immintrin.h>
#endif
#include <utility>
#include <vector>

using namespace xrhip;

namespace {

struct LevelBuf {
    int w = 0, h = 0;
    int istride = 0;   // bytes per padded image row
    int rows = 0;      // padded rows
    uint8_t *img_base = nullptr;
    short2 *der_base = nullptr;
    uint8_t *img = nullptr;   // pixel (0,0)
    short2 *der = nullptr;    // pixel (0,0)
};

// What a request of each kind carries: the argument sets of its kernels, built by the owning context exactly as for a launch of its own
struct PrePayload {
    bool with_upload = false;   // the frame's copy into HBM travels with its preprocessing (grouped contexts: one request per frame)
    UploadArgs up;
    ClaheLutArgs lut;
    PyrAArgs pa;
    PyrBArgs pb;
};
struct DetectPayload {
    HarrisArgs hr;
    HarrisNmsArgs nms;
    HarrisSelectArgs sel;
    const uint8_t *mask = nullptr;   // the image's effective mask: the masked Harris kernels run (never in a group's batch)
};
struct TrackPayload {
    LkTrackArgs lk;
    int n_inline = 0;       // > 0: `inl` holds the points as floats (the kernel's own conversion), for a launch that carries this entry alone
    LkInlinePoints inl;
    bool detect = false;   // the Harris pass of the target image rides behind the tracking launch (xrhip_image_prefetch_detect)
    DetectPayload det;
};

}   // namespace

struct xrhip_klt {
    int device = 0;
    int w = 0, h = 0, max_points = 0;
    hipStream_t stream = nullptr;
    // instance group (group.hip.h): when set, the per-frame launches travel as requests -- one outstanding request of a kind per context
    xrhip_group *group = nullptr;
    GroupRequest rq_upload, rq_pre, rq_track, rq_detect;
    UploadArgs a_upload;
    PrePayload a_pre;
    TrackPayload a_track;
    DetectPayload a_detect;
    int uploads_unsynced = 0;   // grouped: uploads since the last point the KLT queue is known to have drained (pinned ring safety)
    bool upload_pending = false;   // grouped: a_upload describes a copy that has not been submitted yet (xrhip_image_preprocess takes it along)
    // scratch shared by the images of this sequence
    uint8_t *lut = nullptr;          // tiles*256
    int lut_tiles = 0;
    // device undistortion (k_undistort): packed 1/32-pixel map [h][w][2] and the frame as the camera recorded it
    uint32_t *undist_map = nullptr;
    uint8_t *undist_src = nullptr;
    bool have_undist = false;
    // Host frames go through a small ring of pinned buffers: the caller's (pageable) buffer is copied into the next slot and
    // the DMA to HBM is queued on the stream -- the upload call returns after the memcpy, the preprocessing kernels are ordered
    // behind the DMA by the stream.  (hipMemcpy2DAsync from pageable memory stages and waits inside the call: 73 us per
    // 752x480 frame against ~25 for the memcpy, measured as the difference to device-resident input, round 3.)
    static constexpr int UP_SLOTS = 3;
    uint8_t *up_buf[UP_SLOTS] = {nullptr, nullptr, nullptr};
    size_t up_cap = 0;   // bytes per slot
    hipEvent_t up_done[UP_SLOTS] = {nullptr, nullptr, nullptr};
    bool up_busy[UP_SLOTS] = {false, false, false};
    int up_next = 0;
    bool fused_pyramid = true;       // xrhip_debug_set_fused_pyramid / XRHIP_NO_FUSED_PYRAMID: the five-launch path (A/B, parity)
    float *resp = nullptr;           // w*h Harris response
    int *max_key = nullptr;          // 1 int (+ candidate counter next to it)
    int *cand_count = nullptr;
    unsigned *sel_hist = nullptr;    // SEL_BINS counters: k_harris_nms fills them, k_harris_select reads and clears them
    HarrisCand *cand = nullptr;
    int cand_cap = 0;
    HarrisCand *h_cand = nullptr;    // pinned
    int *h_count = nullptr;          // pinned (2 ints)
    HarrisCand *h_top = nullptr;     // pinned, device-mapped: the strongest candidates (k_harris_select)
    SelectHeader *h_sel = nullptr;   // pinned, device-mapped
    int top_cap = SEL_SORT;   // everything the selection kernel can hand over in visiting order
    int sel_seq = 0;
    // track scratch
    int pts_cap = 0;
    // zero-copy point block of xrhip_image_track (pinned, device-mapped): curr | next | status, + completion mailbox
    char *h_pts = nullptr;
    int h_pts_cap = 0;
    unsigned *d_done = nullptr;      // device counter of finished wavefronts (monotonic)
    unsigned done_base = 0;
    int *h_trk_seq = nullptr;        // pinned
    int trk_seq = 0;
    double2 *d_curr = nullptr, *d_next = nullptr;
    uint8_t *d_status = nullptr;
    float2 *d_fprev = nullptr, *d_fnext = nullptr;
    LkCounters *d_counters = nullptr;
    LkCounters *h_counters = nullptr;   // pinned
    // profiling: event pairs are recorded on the stream without synchronising and
    // resolved lazily in xrhip_klt_get_stats(), so timing runs inside the timed region
    bool profiling = false;
    struct Pending {
        hipEvent_t e0, e1;
        int cat;
    };
    std::vector<Pending> pending;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> free_events;
    xrhip_klt_stats stats{};
    // tracking view (xrhip_image_render_view): nothing of it exists before the first render of this context
    uint32_t *view_owner = nullptr;   // w*h owner words
    uint8_t *view_out = nullptr;      // w*h*4: the rendered rows on their way to a host destination
    char *view_stage = nullptr;       // pinned, device-mapped: segments | markers | palette of the render in flight
    size_t view_stage_cap = 0;
    hipEvent_t view_done = nullptr;   // the last render has read the staging block
    bool view_busy = false;
    hipEvent_t view_t0 = nullptr, view_t1 = nullptr;   // xrhip_debug_view_timing
    bool view_timing = false;
    double view_ms = 0;
    long long view_n = 0;
    // frames larger than the plane (xrhip_image_upload_scaled): the crop of a host frame in HBM, where k_upload_scaled reads it.
    // Nothing of it exists before the first scaled (or Bayer) upload of a host frame.  A packed mosaic or scaled packed frame (host
    // or HBM) has its 8-bit samples unpacked into it (upload_packed_into).
    uint8_t *scale_src = nullptr;
    size_t scale_cap = 0;
    // Bayer mosaics (XRHIP_PIXFMT_BAYER_*): a host mosaic is staged in scale_src as well (k_upload_bayer reads it there); a scaled one
    // is demosaiced into this cw x ch gray scratch, which k_upload_scaled then reads.  Allocated by the first scaled Bayer frame.
    uint8_t *bayer_gray = nullptr;
    size_t bayer_gray_cap = 0;
    // turned and mirrored frames (xrhip_klt_set_orientation): o = r + 4 f; the frame's gray plane in the source's orientation (w x h, or
    // h x w for odd r), which k_orient turns into the plane.  Allocated by the first frame uploaded with a non-zero orientation.
    int orient = 0;
    uint8_t *orient_src = nullptr;
    hipEvent_t span_t0 = nullptr, span_t1 = nullptr;   // xrhip_debug_stream_span
    // LK parameters (xrhip_klt_set_lk_params): at the reference's values, with the switch off, the specialised kernels run
    xrhip_lk_params lk{XRHIP_KLT_WIN, XRHIP_KLT_LEVELS - 1, 30, 0.01};
    bool force_general = false;   // xrhip_debug_force_general_lk
    int n_images = 0;             // images alive: their pyramid storage is sized by lk.max_level
    // masks (xrhip_klt_set_mask / xrhip_image_set_mask): nothing of it exists before the first mask of this context
    uint8_t *mask_static = nullptr;   // w*h bytes 0 / 1 in HBM
    bool static_on = false;
    bool mask_used = false;           // an image of this context has been handed a per-frame mask: the context stays out of groups
};

struct xrhip_image {
    xrhip_klt *ctx = nullptr;
    uint8_t *raw = nullptr;    // w*h, unpadded upload target (CLAHE input)
    bool have_raw = false;
    bool have_pyramid = false;
    bool want_detect = false;   // xrhip_image_prefetch_detect: queue the Harris pass behind the next tracking launch
    int detect_seq = 0;         // != 0: the Harris pass of this image is in flight / done under that sequence number
    int levels = KLT_LEVELS;    // ctx->lk.max_level + 1 when the image was created
    LevelBuf lv[KLT_MAX_LEVELS];
    // effective mask = static && per-frame (w*h bytes 0 / 1 in HBM; allocated by the image's first masked frame)
    uint8_t *mask = nullptr;
    bool mask_on = false;         // `mask` holds this frame's effective mask
    bool mask_resolved = false;   // this frame's effective mask is decided (an upload resets it; resolve_mask decides)
};

static PyrView make_view(const xrhip_image *img) {
    PyrView v;
    for (int l = 0; l < KLT_LEVELS; ++l) {
        v.lv[l].img = img->lv[l].img;
        v.lv[l].der = img->lv[l].der;
        v.lv[l].w = img->lv[l].w;
        v.lv[l].h = img->lv[l].h;
        v.lv[l].istride = img->lv[l].istride;
        v.lv[l].pstride = img->lv[l].istride;
    }
    return v;
}

static bool lk_is_default(const xrhip_lk_params &p) {
    return p.win == XRHIP_KLT_WIN && p.max_level == XRHIP_KLT_LEVELS - 1 && p.max_count == 30 && p.epsilon == 0.01;
}
// the kernels with runtime parameters run for this context (klt_kernels.hip.h, "LK with runtime parameters")
static bool lk_general(const xrhip_klt *c) { return c->force_general || !lk_is_default(c->lk); }
static PyrViewG make_view_g(const xrhip_image *img) {
    PyrViewG v;
    std::memset(&v, 0, sizeof(v));
    for (int l = 0; l < img->levels; ++l) {
        v.lv[l].img = img->lv[l].img;
        v.lv[l].der = img->lv[l].der;
        v.lv[l].w = img->lv[l].w;
        v.lv[l].h = img->lv[l].h;
        v.lv[l].istride = img->lv[l].istride;
        v.lv[l].pstride = img->lv[l].istride;
    }
    return v;
}
static LkParams lk_device_params(const xrhip_klt *c) {
    return LkParams{c->lk.win, c->lk.max_level + 1, c->lk.max_count, c->lk.epsilon * c->lk.epsilon};
}

static int ensure_points(xrhip_klt *c, int n) {
    if (n <= c->pts_cap) return XRHIP_OK;
    int cap = std::max(n, std::max(256, c->pts_cap * 2));
    hipFree(c->d_curr);
    hipFree(c->d_next);
    hipFree(c->d_status);
    hipFree(c->d_fprev);
    hipFree(c->d_fnext);
    c->d_curr = c->d_next = nullptr;
    c->d_status = nullptr;
    c->d_fprev = c->d_fnext = nullptr;
    XR_HIP(hipMalloc(&c->d_curr, sizeof(double2) * cap));
    XR_HIP(hipMalloc(&c->d_next, sizeof(double2) * cap));
    XR_HIP(hipMalloc(&c->d_status, cap));
    XR_HIP(hipMalloc(&c->d_fprev, sizeof(float2) * cap));
    XR_HIP(hipMalloc(&c->d_fnext, sizeof(float2) * cap));
    c->pts_cap = cap;
    return XRHIP_OK;
}

enum { CAT_PRE = 0, CAT_TRACK = 1, CAT_DETECT = 2 };

static int resolve_pending(xrhip_klt *c) {
    if (c->pending.empty()) return XRHIP_OK;
    XR_HIP(hipStreamSynchronize(c->stream));
    for (auto &p : c->pending) {
        float ms = 0.f;
        XR_HIP(hipEventElapsedTime(&ms, p.e0, p.e1));
        if (p.cat == CAT_PRE) c->stats.ms_preprocess += ms;
        else if (p.cat == CAT_TRACK) c->stats.ms_track += ms;
        else c->stats.ms_detect += ms;
        c->free_events.emplace_back(p.e0, p.e1);
    }
    c->pending.clear();
    return XRHIP_OK;
}

struct ProfScope {
    xrhip_klt *c;
    int cat;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ProfScope(xrhip_klt *c_, int cat_) : c(c_), cat(cat_) {
        if (!c->profiling || c->group) return;   // grouped: the launch is the group's (xrhip_group_get_stats times the batches)
        if (c->pending.size() >= 8192) resolve_pending(c);
        if (!c->free_events.empty()) {
            e0 = c->free_events.back().first;
            e1 = c->free_events.back().second;
            c->free_events.pop_back();
        } else {
            hipEventCreate(&e0);
            hipEventCreate(&e1);
        }
        hipEventRecord(e0, c->stream);
    }
    void finish() {
        if (c->profiling && e0 && !c->group) {
            hipEventRecord(e1, c->stream);
            c->pending.push_back({e0, e1, cat});
        }
        if (cat == CAT_PRE) c->stats.n_preprocess++;
        else if (cat == CAT_TRACK) c->stats.n_track++;
        else c->stats.n_detect++;
    }
};

// ---------------------------------------------------------------------------------------------- batched launches
// One function per request kind turns n requests into launches on `s`, XB entries per launch (blockIdx.z = entry).  A context
// that launches for itself calls the same function with its one request and its own stream.
template <class Args, class Fill> static void for_chunks(int n, Fill fill) {
    for (int base = 0; base < n; base += XB) {
        const int m = std::min(XB, n - base);
        Batch<Args> b;
        std::memset(&b, 0, sizeof(b));
        fill(b, base, m);
    }
}

static int launch_upload_batch(GroupRequest **r, int n, hipStream_t s, hipStream_t) {
    for_chunks<UploadArgs>(n, [&](Batch<UploadArgs> &b, int base, int m) {
        size_t most = 0;
        for (int i = 0; i < m; ++i) {
            b.e[i] = *static_cast<const UploadArgs *>(r[base + i]->payload);
            most = std::max(most, (size_t)b.e[i].w * b.e[i].h);
        }
        const int blocks = (int)std::min<size_t>((most / 16 + 255) / 256, 64);   // 64 workgroups per frame saturate the host link
        hipLaunchKernelGGL(k_upload, dim3(std::max(blocks, 1), 1, m), dim3(256), 0, s, b);
    });
    XR_HIP(hipGetLastError());
    return XRHIP_OK;
}

static int launch_preprocess_batch(GroupRequest **r, int n, hipStream_t s, hipStream_t) {
    for (int base = 0; base < n; base += XB) {
        const int m = std::min(XB, n - base);
        Batch<ClaheLutArgs> bl;
        Batch<PyrAArgs> ba;
        Batch<PyrBArgs> bb;
        std::memset(&bl, 0, sizeof(bl));
        std::memset(&ba, 0, sizeof(ba));
        std::memset(&bb, 0, sizeof(bb));
        int gl = 1, ga = 1, gb = 1;
        Batch<UploadArgs> bu;
        std::memset(&bu, 0, sizeof(bu));
        size_t most = 0;
        for (int i = 0; i < m; ++i) {
            const PrePayload &p = *static_cast<const PrePayload *>(r[base + i]->payload);
            if (p.with_upload) {
                bu.e[i] = p.up;
                most = std::max(most, (size_t)p.up.w * p.up.h);
            }
        }
        if (most) hipLaunchKernelGGL(k_upload, dim3((int)std::max<size_t>(1, std::min<size_t>((most / 16 + 255) / 256, 64)), 1, m), dim3(256), 0, s, bu);
        for (int i = 0; i < m; ++i) {
            const PrePayload &p = *static_cast<const PrePayload *>(r[base + i]->payload);
            bl.e[i] = p.lut;
            ba.e[i] = p.pa;
            bb.e[i] = p.pb;
            gl = std::max(gl, p.lut.tiles);
            ga = std::max(ga, p.pa.blocks);
            gb = std::max(gb, p.pb.blocks);
        }
        hipLaunchKernelGGL(k_clahe_lut, dim3(gl, 1, m), dim3(CL_THREADS), 0, s, bl);
        hipLaunchKernelGGL(k_pyr_a, dim3(ga, 1, m), dim3(PF_THREADS), 0, s, ba);
        hipLaunchKernelGGL(k_pyr_b, dim3(gb, 1, m), dim3(PF_THREADS), 0, s, bb);
    }
    XR_HIP(hipGetLastError());
    return XRHIP_OK;
}

static void launch_detect_chunk(const DetectPayload *const *d, int m, hipStream_t s) {
    Batch<HarrisArgs> bh;
    Batch<HarrisNmsArgs> bn;
    Batch<HarrisSelectArgs> bs;
    std::memset(&bh, 0, sizeof(bh));
    std::memset(&bn, 0, sizeof(bn));
    std::memset(&bs, 0, sizeof(bs));
    int gx = 1, gy = 1;
    for (int i = 0; i < m; ++i) {
        bh.e[i] = d[i]->hr;
        bn.e[i] = d[i]->nms;
        bs.e[i] = d[i]->sel;
        gx = std::max(gx, d[i]->hr.gx);
        gy = std::max(gy, d[i]->hr.gy);
    }
    if (m == 1 && d[0]->mask) {   // an image with an effective mask (its context launches for itself): the masked maximum and NMS
        hipLaunchKernelGGL(k_harris_m, dim3(gx, gy, 1), dim3(256), 0, s, d[0]->hr, d[0]->mask);
        hipLaunchKernelGGL(k_harris_nms_m, dim3(gx, gy, 1), dim3(256), 0, s, d[0]->nms, d[0]->mask);
    } else {
        hipLaunchKernelGGL(k_harris, dim3(gx, gy, m), dim3(256), 0, s, bh);
        hipLaunchKernelGGL(k_harris_nms, dim3(gx, gy, m), dim3(256), 0, s, bn);
    }
    hipLaunchKernelGGL(k_harris_select, dim3(1, 1, m), dim3(1024), SEL_LDS_BYTES, s, bs);
}

static int launch_detect_batch(GroupRequest **r, int n, hipStream_t s, hipStream_t) {
    for (int base = 0; base < n; base += XB) {
        const int m = std::min(XB, n - base);
        const DetectPayload *d[XB];
        for (int i = 0; i < m; ++i) d[i] = static_cast<const DetectPayload *>(r[base + i]->payload);
        launch_detect_chunk(d, m, s);
    }
    XR_HIP(hipGetLastError());
    return XRHIP_OK;
}

static int launch_track_batch(GroupRequest **r, int n, hipStream_t s, hipStream_t side) {
    for (int base = 0; base < n; base += XB) {
        const int m = std::min(XB, n - base);
        if (m == 1 && n == 1) {   // a lone entry whose points fit the argument block: no read of the pinned list at kernel start
            const TrackPayload *tp1 = static_cast<const TrackPayload *>(r[base]->payload);
            if (tp1->n_inline > 0) {
                hipLaunchKernelGGL(k_lk_track_inl, dim3(std::max(1, tp1->lk.n), 1, 1), dim3(LK_THREADS), 0, s, tp1->lk, tp1->inl);
                continue;
            }
        }
        Batch<LkTrackArgs> b;
        std::memset(&b, 0, sizeof(b));
        int most = 1;
        for (int i = 0; i < m; ++i) {
            b.e[i] = static_cast<const TrackPayload *>(r[base + i]->payload)->lk;
            most = std::max(most, b.e[i].n);
        }
        hipLaunchKernelGGL(k_lk_track, dim3(most, 1, m), dim3(LK_THREADS), 0, s, b);
    }
    XR_HIP(hipGetLastError());
    // The Harris passes of the target images do not depend on the tracking result: right behind the tracking launch -- on the queue's
    // side stream when there is one (ordered behind this batch by an event: they read the pyramids the stream has built), so that
    // the queue's next batch does not wait for three kernels nobody needs before the tracks have been digested.
    const DetectPayload *d[XB];
    int nd = 0;
    bool any = false;
    for (int i = 0; i < n && !any; ++i) any = static_cast<const TrackPayload *>(r[i]->payload)->detect;
    if (!any) return XRHIP_OK;
    hipStream_t ds = s;
    if (side) {
        static thread_local hipEvent_t fork[8] = {nullptr};
        static thread_local unsigned fork_next = 0;
        hipEvent_t &e = fork[fork_next++ & 7];
        if (!e) XR_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        XR_HIP(hipEventRecord(e, s));
        XR_HIP(hipStreamWaitEvent(side, e, 0));
        ds = side;
    }
    for (int i = 0; i < n; ++i) {
        const TrackPayload *t = static_cast<const TrackPayload *>(r[i]->payload);
        if (!t->detect) continue;
        d[nd++] = &t->det;
        if (nd == XB) {
            launch_detect_chunk(d, nd, ds);
            nd = 0;
        }
    }
    if (nd) launch_detect_chunk(d, nd, ds);
    XR_HIP(hipGetLastError());
    return XRHIP_OK;
}

namespace {
struct RegisterKltLaunchers {
    RegisterKltLaunchers() {
        group_register(GK_UPLOAD, launch_upload_batch);
        group_register(GK_PREPROCESS, launch_preprocess_batch);
        group_register(GK_TRACK, launch_track_batch);
        group_register(GK_DETECT, launch_detect_batch);
    }
} g_register_klt_launchers;
}   // namespace

// a request of `kind` with `payload`: to the group's queue, or launched here and now on the context's own stream
static int klt_issue(xrhip_klt *c, GroupRequest &rq, int kind, void *payload, GroupLaunchFn fn) {
    rq.kind = kind;
    rq.owner = c;
    rq.payload = payload;
    if (c->group) return group_submit(c->group, GQ_KLT, &rq);
    GroupRequest *one = &rq;
    return fn(&one, 1, c->stream, nullptr);
}
static hipStream_t klt_stream(const xrhip_klt *c) { return c->group ? group_stream(c->group, GQ_KLT) : c->stream; }
// a frame copy that was waiting for its preprocessing request goes out on its own (something else is about to read the plane)
static int flush_upload(xrhip_klt *c) {
    if (!c->upload_pending) return XRHIP_OK;
    c->upload_pending = false;
    return klt_issue(c, c->rq_upload, GK_UPLOAD, &c->a_upload, launch_upload_batch);
}
// fn(stream) in the context's launch order (rare, un-batched paths), then wait for everything issued so far
static int klt_run_sync(xrhip_klt *c, std::function<int(hipStream_t)> fn) {
    {
        const int rc = flush_upload(c);
        if (rc) return rc;
    }
    if (!c->group) {
        int rc = fn(c->stream);
        if (rc) return rc;
        XR_HIP(hipStreamSynchronize(c->stream));
        return XRHIP_OK;
    }
    int rc = group_call(c->group, GQ_KLT, c, std::move(fn));
    if (rc) return rc;
    XR_HIP(hipStreamSynchronize(group_stream(c->group, GQ_KLT)));
    c->uploads_unsynced = 0;
    return XRHIP_OK;
}
static int klt_run(xrhip_klt *c, std::function<int(hipStream_t)> fn) {   // same without the wait
    {
        const int rc = flush_upload(c);
        if (rc) return rc;
    }
    if (!c->group) return fn(c->stream);
    return group_call(c->group, GQ_KLT, c, std::move(fn));
}

extern "C" {

int xrhip_klt_join_group(xrhip_klt *c, xrhip_group *g) {
    if (!c) return xr_fail(XRHIP_EINVAL, "xrhip_klt_join_group: null context");
    if (c->group == g) return XRHIP_OK;
    if (g && group_device(g) != c->device)
        return xr_fail(XRHIP_EINVAL, "xrhip_klt_join_group: the context and the group live on different devices");
    if (g && lk_general(c))
        return xr_fail(XRHIP_ESTATE, "xrhip_klt_join_group: a context with non-default LK parameters (xrhip_klt_set_lk_params) cannot join a group");
    if (g && (c->static_on || c->mask_used))
        return xr_fail(XRHIP_ESTATE, "xrhip_klt_join_group: a context with a mask (xrhip_klt_set_mask / xrhip_image_set_mask) cannot join a group");
    // whatever the context has queued so far completes where it was queued
    {
        const int rc = flush_upload(c);
        if (rc) return rc;
    }
    if (c->group) {
        int rc = group_drain(c->group, GQ_KLT, c);
        if (rc) return rc;
        group_gate_unregister(c->group, c);
        group_member_remove(c->group, true);
    } else {
        XR_HIP(hipStreamSynchronize(c->stream));
    }
    c->group = g;
    c->uploads_unsynced = 0;
    for (int i = 0; i < xrhip_klt::UP_SLOTS; ++i) c->up_busy[i] = false;
    if (g) {
        group_member_add(g, true);
        group_gate_register(g, c);
    }
    return XRHIP_OK;
}

int xrhip_klt_frame_gate(xrhip_klt *c) {
    if (!c) return xr_fail(XRHIP_EINVAL, "xrhip_klt_frame_gate: null context");
    if (c->group) group_gate_arrive(c->group, c);
    return XRHIP_OK;
}
int xrhip_klt_group_busy(xrhip_klt *c, int busy) {
    if (!c) return xr_fail(XRHIP_EINVAL, "xrhip_klt_group_busy: null context");
    if (c->group) group_gate_busy(c->group, c, busy != 0);
    return XRHIP_OK;
}

int xrhip_klt_create(int width, int height, int max_points, xrhip_klt **out) {
    // (the tracker wants 64 pixels a side -- xrhip_image_preprocess; a frame of 32 can still be uploaded and viewed)
    if (!out || width < 32 || height < 32 || max_points < 0) return xr_fail(XRHIP_EINVAL, "xrhip_klt_create: bad arguments");
    int rc = xr_require_device();
    if (rc) return rc;
    xrhip_klt *c = new xrhip_klt();
    hipGetDevice(&c->device);
    c->w = width;
    c->h = height;
    c->max_points = max_points;
    c->fused_pyramid = std::getenv("XRHIP_NO_FUSED_PYRAMID") == nullptr;
    XR_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->lut_tiles = 0;
    XR_HIP(hipMalloc(&c->resp, sizeof(float) * (size_t)width * height));
    XR_HIP(hipMalloc(&c->max_key, sizeof(int) * 2));
    c->cand_count = c->max_key + 1;
    {   // running maximum (as an order-preserving int key) and candidate counter: k_harris_select leaves them reset for the next pass
        const int init[2] = {(int)0x80000000, 0};
        XR_HIP(hipMemcpy(c->max_key, init, sizeof(init), hipMemcpyHostToDevice));
    }
    c->cand_cap = width * height / 2;
    XR_HIP(hipFuncSetAttribute((const void *)k_harris_select, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SEL_LDS_BYTES));
    XR_HIP(hipMalloc(&c->cand, sizeof(HarrisCand) * (size_t)c->cand_cap));
    XR_HIP(hipMalloc(&c->sel_hist, sizeof(unsigned) * SEL_BINS));
    XR_HIP(hipMemset(c->sel_hist, 0, sizeof(unsigned) * SEL_BINS));
    XR_HIP(hipHostMalloc(&c->h_cand, sizeof(HarrisCand) * (size_t)c->cand_cap, hipHostMallocDefault));
    XR_HIP(hipHostMalloc(&c->h_count, sizeof(int) * 2, hipHostMallocDefault));
    XR_HIP(hipHostMalloc(&c->h_top, sizeof(HarrisCand) * (size_t)c->top_cap, hipHostMallocDefault));
    XR_HIP(hipHostMalloc(&c->h_trk_seq, 64, hipHostMallocDefault));
    *c->h_trk_seq = 0;
    XR_HIP(hipMalloc(&c->d_done, sizeof(unsigned)));
    XR_HIP(hipMemset(c->d_done, 0, sizeof(unsigned)));
    XR_HIP(hipHostMalloc(&c->h_sel, sizeof(SelectHeader), hipHostMallocDefault));
    std::memset(c->h_sel, 0, sizeof(SelectHeader));
    XR_HIP(hipMalloc(&c->d_counters, sizeof(LkCounters)));
    XR_HIP(hipMemset(c->d_counters, 0, sizeof(LkCounters)));
    XR_HIP(hipHostMalloc(&c->h_counters, sizeof(LkCounters), hipHostMallocDefault));
    c->up_cap = (size_t)width * height;
    for (int i = 0; i < xrhip_klt::UP_SLOTS; ++i) {
        XR_HIP(hipHostMalloc(&c->up_buf[i], (size_t)width * height, hipHostMallocDefault));   // (grows with the first colour frame)
        XR_HIP(hipEventCreateWithFlags(&c->up_done[i], hipEventDisableTiming));
    }
    rc = ensure_points(c, std::max(256, max_points * 2));
    if (rc) return rc;
    *out = c;
    return XRHIP_OK;
}

void xrhip_klt_destroy(xrhip_klt *c) {
    if (!c) return;
    hostprof_dump();
    if (c->group) xrhip_klt_join_group(c, nullptr);
    hipStreamSynchronize(c->stream);
    hipFree(c->lut);
    hipFree(c->undist_map);
    hipFree(c->undist_src);
    hipFree(c->resp);
    hipFree(c->max_key);
    hipFree(c->cand);
    hipFree(c->sel_hist);
    hipHostFree(c->h_cand);
    hipHostFree(c->h_count);
    hipHostFree(c->h_top);
    hipHostFree(c->h_trk_seq);
    hipHostFree(c->h_pts);
    hipFree(c->d_done);
    hipHostFree(c->h_sel);
    hipFree(c->d_curr);
    hipFree(c->d_next);
    hipFree(c->d_status);
    hipFree(c->d_fprev);
    hipFree(c->d_fnext);
    hipFree(c->d_counters);
    hipHostFree(c->h_counters);
    hipFree(c->view_owner);
    hipFree(c->view_out);
    hipHostFree(c->view_stage);
    if (c->view_done) hipEventDestroy(c->view_done);
    if (c->view_t0) hipEventDestroy(c->view_t0);
    if (c->view_t1) hipEventDestroy(c->view_t1);
    hipFree(c->scale_src);
    hipFree(c->bayer_gray);
    hipFree(c->orient_src);
    hipFree(c->mask_static);
    if (c->span_t0) hipEventDestroy(c->span_t0);
    if (c->span_t1) hipEventDestroy(c->span_t1);
    for (int i = 0; i < xrhip_klt::UP_SLOTS; ++i) {
        hipHostFree(c->up_buf[i]);
        if (c->up_done[i]) hipEventDestroy(c->up_done[i]);
    }
    for (auto &p : c->pending) {
        hipEventDestroy(p.e0);
        hipEventDestroy(p.e1);
    }
    for (auto &p : c->free_events) {
        hipEventDestroy(p.first);
        hipEventDestroy(p.second);
    }
    hipStreamDestroy(c->stream);
    delete c;
}

int xrhip_image_create(xrhip_klt *c, xrhip_image **out) {
    if (!c || !out) return xr_fail(XRHIP_EINVAL, "xrhip_image_create: null argument");
    xrhip_image *im = new xrhip_image();
    im->ctx = c;
    im->levels = c->lk.max_level + 1;
    XR_HIP(hipMalloc(&im->raw, (size_t)c->w * c->h));
    int w = c->w, h = c->h;
    for (int l = 0; l < im->levels; ++l) {
        LevelBuf &L = im->lv[l];
        L.w = w;
        L.h = h;
        L.istride = (KLT_PADX + w + KLT_PAD + 3 + 63) / 64 * 64;   // + 3: k_lk_track stages rows as whole dwords
        L.rows = h + 2 * KLT_PAD;
        XR_HIP(hipMalloc(&L.img_base, (size_t)L.rows * L.istride));
        XR_HIP(hipMalloc(&L.der_base, sizeof(short2) * (size_t)L.rows * L.istride));
        // derivative borders are BORDER_CONSTANT(0) and never rewritten
        XR_HIP(hipMemsetAsync(L.der_base, 0, sizeof(short2) * (size_t)L.rows * L.istride, c->stream));
        XR_HIP(hipMemsetAsync(L.img_base, 0, (size_t)L.rows * L.istride, c->stream));
        L.img = L.img_base + (size_t)KLT_PAD * L.istride + KLT_PADX;
        L.der = L.der_base + (size_t)KLT_PAD * L.istride + KLT_PADX;
        w = (w + 1) / 2;
        h = (h + 1) / 2;
    }
    XR_HIP(hipStreamSynchronize(c->stream));   // (the planes are cleared before any queue -- the context's or a group's -- can reach them)
    c->n_images++;
    *out = im;
    return XRHIP_OK;
}

void xrhip_image_destroy(xrhip_image *im) {
    if (!im) return;
    // a grouped upload that nobody has submitted yet and that writes THIS plane: dropped, not submitted later into freed memory
    // (the context's teardown flushes whatever is pending)
    if (im->ctx->upload_pending && im->ctx->a_upload.dst == im->raw) im->ctx->upload_pending = false;
    if (im->ctx->group) group_drain(im->ctx->group, GQ_KLT, im->ctx);
    hipStreamSynchronize(im->ctx->stream);
    hipFree(im->raw);
    hipFree(im->mask);
    for (int l = 0; l < im->levels; ++l) {
        hipFree(im->lv[l].img_base);
        hipFree(im->lv[l].der_base);
    }
    im->ctx->n_images--;
    delete im;
}

// memcpy into the pinned slot with streaming stores where the CPU has AVX2: the slot is written once and read by the DMA engine,
// never by this core -- non-temporal stores skip the read-for-ownership of every destination line (a 752x480 frame: 360 KB).
#if defined(__x86_64__)
__attribute__((target("avx2"))) static void copy_stream_avx2(uint8_t *dst, const uint8_t *src, size_t n) {
    size_t i = 0;
    while (i < n && (reinterpret_cast<uintptr_t>(dst + i) & 31)) {
        dst[i] = src[i];
        ++i;
    }
    for (; i + 128 <= n; i += 128) {
        const __m256i a = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i));
        const __m256i b = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i + 32));
        const __m256i c2 = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i + 64));
        const __m256i d = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i + 96));
        _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i), a);
        _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i + 32), b);
        _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i + 64), c2);
        _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i + 96), d);
    }
    _mm_sfence();
    for (; i < n; ++i) dst[i] = src[i];
}
#endif
static void copy_to_pinned(uint8_t *dst, const uint8_t *src, size_t n) {
#if defined(__x86_64__)
    static const bool avx2 = __builtin_cpu_supports("avx2");
    if (avx2 && n >= 4096) {
        copy_stream_avx2(dst, src, n);
        return;
    }
#endif
    std::memcpy(dst, src, n);
}

// ------------------------------------------------------------------------------------------------------------ frames on their way in
// What an upload entry point was handed.  Every xrhip_image_upload* builds one and calls upload_frame: the frame is validated once,
// goes one way into the plane (im->raw, or undist_src when the undistortion remap follows) and the image's state is reset in one place.
struct FrameSource {
    const uint8_t *pixels;
    int stride;
    xrh::PixelFormat pf;   // (default: 8-bit gray)
    bool on_device;        // pixels lie in HBM and are read where they lie
    const xrhip_frame_geometry *geo;
    bool scaled;           // larger than the plane: the crop of `geo` is area-averaged down (geo == nullptr is then an error)
    int pw = 0, ph = 0;    // the plane as the frame sees it (upload_frame): w x h, or h x w under an orientation with odd r
};
static FrameSource frame_source(const void *pixels, int stride, int on_device, const xrhip_frame_geometry *geo = nullptr, bool scaled = false) {
    return FrameSource{static_cast<const uint8_t *>(pixels), stride, xrh::PixelFormat(), on_device != 0, geo, scaled};
}
// the older entry points' `channels`: 1 GRAY8, 3 BGR8, 4 BGRA8 (nullptr, or what is wrong: as describe_pixel_format)
static const char *describe_channels(int channels, xrh::PixelFormat &pf) {
    if (channels != 1 && channels != 3 && channels != 4) return "channels must be 1, 3 (BGR) or 4 (BGRA)";
    return xrh::describe_pixel_format(channels == 1 ? XRHIP_PIXFMT_GRAY8 : channels == 3 ? XRHIP_PIXFMT_BGR8 : XRHIP_PIXFMT_BGRA8, 0, 0, pf);
}
static int frame_fail(int code, const char *who, const char *why) { return xr_fail(code, (std::string(who) + ": " + why).c_str()); }
// bad_format: what describe_pixel_format / describe_channels said about the entry point's format arguments
static int check_frame(const char *who, const xrhip_image *im, const FrameSource &s, const char *bad_format) {
    if (!im) return frame_fail(XRHIP_EINVAL, who, "img is null");
    if (!s.pixels) return frame_fail(XRHIP_EINVAL, who, "pixels is null");
    if (bad_format) return frame_fail(XRHIP_EINVAL, who, bad_format);
    if (s.scaled) {
        if (const char *why = xrh::check_frame_geometry(s.geo, s.pw, s.ph, s.pf, s.stride))
            return frame_fail(XRHIP_EINVAL, who, s.pw == im->ctx->w ? why : (std::string(why) + " (orientation: the frame is turned, the crop must cover height x width)").c_str());
    } else if ((long long)s.stride < s.pf.row_bytes(s.pw)) {
        if (s.pf.packing) return frame_fail(XRHIP_EINVAL, who, "stride_bytes < the packed bytes of a row");
        return frame_fail(XRHIP_EINVAL, who, s.pw == im->ctx->w ? "stride_bytes < width * bytes per pixel"
                                                                 : "stride_bytes < height * bytes per pixel (orientation: the frame is height x width in memory)");
    }
    return XRHIP_OK;
}
// UploadArgs::fmt / ScaleArgs::fmt of a format (UPF_*, klt_kernels.hip.h); 0 for GRAY8 without a range flag, BGR8 and BGRA8
static int upf_word(const xrh::PixelFormat &pf) {
    return (pf.bpp == 2 ? (int)pf.shift | (pf.mask == 0xffu ? UPF_LOW_BYTE : 0) : 0) | (pf.rgb ? UPF_RGB : 0) | (pf.limited ? UPF_LIMITED : 0);
}

// Before a buffer the GPU may still be reading is freed to grow: everything the context has issued so far completes
static int wait_before_growth(xrhip_klt *c) {
    if (!c->group) {
        XR_HIP(hipStreamSynchronize(c->stream));
        return XRHIP_OK;
    }
    int rc = flush_upload(c);
    if (rc) return rc;
    rc = group_drain(c->group, GQ_KLT, c);
    if (rc) return rc;
    c->uploads_unsynced = 0;
    return XRHIP_OK;
}
// The pinned slots hold a gray frame until the first larger frame arrives: a gray-only caller never pays for the colour size.
static int ensure_slot_bytes(xrhip_klt *c, size_t bytes) {
    if (bytes <= c->up_cap) return XRHIP_OK;
    const int rc = wait_before_growth(c);
    if (rc) return rc;
    for (int i = 0; i < xrhip_klt::UP_SLOTS; ++i) {
        hipHostFree(c->up_buf[i]);
        c->up_buf[i] = nullptr;
        c->up_busy[i] = false;
    }
    c->up_cap = 0;
    for (int i = 0; i < xrhip_klt::UP_SLOTS; ++i) XR_HIP(hipHostMalloc(&c->up_buf[i], bytes, hipHostMallocDefault));
    c->up_cap = bytes;
    return XRHIP_OK;
}
// The next pinned slot, large enough and safe to overwrite, filled with `rows` rows of `row` bytes (`stride` apart at `src`, packed
// in the slot): the caller's buffer is free on return.  slot_in_flight follows once the slot's reader has been queued.
static int slot_fill(xrhip_klt *c, const uint8_t *src, int stride, size_t row, int rows, int &slot) {
    const int rc = ensure_slot_bytes(c, row * rows);
    if (rc) return rc;
    slot = c->up_next;
    c->up_next = (slot + 1) % xrhip_klt::UP_SLOTS;
    if (c->group) {
        // the slot was read by the upload launched three frames ago; the pipeline has waited for two tracking results since (same
        // queue, in order).  A caller that uploads without ever waiting is held here instead.
        if (c->uploads_unsynced >= xrhip_klt::UP_SLOTS - 1) {
            const int rd = group_drain(c->group, GQ_KLT, c);
            if (rd) return rd;
            c->uploads_unsynced = 0;
        }
    } else if (c->up_busy[slot]) {
        XR_HIP(hipEventSynchronize(c->up_done[slot]));   // three uploads ago: long done unless nothing consumed them
    }
    if ((size_t)stride == row) copy_to_pinned(c->up_buf[slot], src, row * rows);
    else xrh::pack_rows(c->up_buf[slot], src, stride, row, rows);
    return XRHIP_OK;
}
static int slot_in_flight(xrhip_klt *c, int slot) {
    if (c->group) {
        c->uploads_unsynced++;
        return XRHIP_OK;
    }
    XR_HIP(hipEventRecord(c->up_done[slot], c->stream));
    c->up_busy[slot] = true;
    return XRHIP_OK;
}

// A k_upload request.  A group member's is deferred: it is submitted with the frame's preprocessing (xrhip_image_preprocess), or by
// whoever reads the plane first.  A context on its own launches it here and now.
static int queue_upload(xrhip_klt *c, const UploadArgs &a) {
    if (c->group) {
        int rc = group_wait_launched(&c->rq_upload);   // (its argument block is about to be rewritten)
        if (rc) return rc;
        if (c->upload_pending) {   // an earlier frame nobody preprocessed goes out on its own -- and reads the block before it changes
            rc = flush_upload(c);
            if (rc) return rc;
            rc = group_wait_launched(&c->rq_upload);
            if (rc) return rc;
        }
        c->a_upload = a;
        c->upload_pending = true;
        return XRHIP_OK;
    }
    c->a_upload = a;
    return klt_issue(c, c->rq_upload, GK_UPLOAD, &c->a_upload, launch_upload_batch);
}
// A frame of the plane's size into `dst` (s.pw * s.ph, dense).  8-bit gray on a context of its own is a copy: DMA from the pinned slot, or
// device to device.  Everything else is a k_upload request (fmt: UPF_*), which reduces the other formats to gray as it reads -- a host
// frame from the mapped slot, so the plane in HBM is written once and the frame's bytes cross the host link once.
static int upload_into(xrhip_klt *c, const FrameSource &s, uint8_t *dst) {
    const int bpp = s.pf.bpp, fmt = upf_word(s.pf);
    const bool copy = !c->group && bpp == 1 && fmt == 0;
    if (s.on_device) {
        if (!copy) return queue_upload(c, UploadArgs{s.pixels, s.stride, dst, s.pw, s.ph, bpp, fmt});
        XR_HIP(hipMemcpy2DAsync(dst, s.pw, s.pixels, s.stride, s.pw, s.ph, hipMemcpyDeviceToDevice, c->stream));
        return XRHIP_OK;
    }
    const size_t row = (size_t)s.pw * bpp;
    int slot = 0;
    int rc = slot_fill(c, s.pixels, s.stride, row, s.ph, slot);
    if (rc) return rc;
    uint8_t *buf = c->up_buf[slot];
    if (copy) {
        XR_HIP(hipMemcpyAsync(dst, buf, row * s.ph, hipMemcpyHostToDevice, c->stream));
    } else {
        uint8_t *dbuf = nullptr;
        XR_HIP(hipHostGetDevicePointer((void **)&dbuf, buf, 0));
        rc = queue_upload(c, UploadArgs{dbuf, (int)row, dst, s.pw, s.ph, bpp, fmt});
        if (rc) return rc;
    }
    return slot_in_flight(c, slot);
}

// An HBM scratch of the context grown to `bytes` (whatever the context has issued may still be reading the old one)
static int grow_scratch(xrhip_klt *c, uint8_t *&buf, size_t &cap, size_t bytes) {
    if (bytes <= cap) return XRHIP_OK;
    const int rc = wait_before_growth(c);
    if (rc) return rc;
    hipFree(buf);
    buf = nullptr;
    cap = 0;
    XR_HIP(hipMalloc(&buf, bytes));
    cap = bytes;
    return XRHIP_OK;
}
// k_upload_scaled's arguments: the cw x ch crop at `src` (bpp, fmt: as UploadArgs) down to the w x h plane at `dst`
static ScaleArgs scale_args(int w, int h, const uint8_t *src, int stride, int bpp, int fmt, int cw, int ch, uint8_t *dst) {
    ScaleArgs a{};
    a.src = src;
    a.sstride = stride;
    a.dst = dst;
    a.w = w;
    a.h = h;
    a.bpp = bpp;
    a.fmt = fmt;
    a.cw = cw;
    a.ch = ch;
    a.wide = ((uint64_t)w * (uint64_t)cw >> 32) != 0 || ((uint64_t)h * (uint64_t)ch >> 32) != 0;
    return a;
}
static dim3 grid_of_fours(size_t pixels) {   // a lane owns four plane pixels, a block 1024; grid-stride beyond 2048 blocks
    const unsigned n4 = (unsigned)((pixels + 3) / 4);
    return dim3(std::max(1u, std::min((n4 + 255u) / 256u, 2048u)));
}
// The crop of a frame of any pixel format, area-averaged down to the context's plane (k_upload_scaled) on the way in.  A frame in HBM
// is read where it lies.  A host frame: only the crop is staged (rows of cw * bpp bytes, packed) through the pinned slots, which grow
// as they do for colour; the slot is then copied to an HBM scratch and the kernel reads that.  Neighbouring plane pixels share
// source pixels and a plane row's footprint rows are read by several wavefronts, so a kernel reading the mapped slot would fetch
// bytes over the host link more than once unless every repeat hit a cache -- nothing guarantees that for host memory; the copy costs
// one HBM write and read of the crop and makes "once over the link" hold by construction.
// Not part of the shared upload launch: like the undistortion remap it is a launch of its own, in the context's order (a group
// member: on the group's front-end queue, behind a pending upload, which is submitted first).
static int upload_scaled_into(xrhip_klt *c, const FrameSource &s, uint8_t *dst) {
    const int cw = s.geo->crop_width, ch = s.geo->crop_height;
    ScaleArgs a = scale_args(s.pw, s.ph, xrh::crop_origin(s.pixels, s.stride, *s.geo, s.pf.bpp), s.stride, s.pf.bpp, upf_word(s.pf), cw, ch, dst);
    const dim3 grid = grid_of_fours((size_t)s.pw * s.ph);
    const size_t row = (size_t)cw * s.pf.bpp, bytes = row * ch;
    const uint8_t *staged = nullptr;   // host frame: the slot that holds the crop
    int slot = 0;
    if (!s.on_device) {
        int rc = grow_scratch(c, c->scale_src, c->scale_cap, bytes);
        if (rc) return rc;
        rc = slot_fill(c, a.src, s.stride, row, ch, slot);
        if (rc) return rc;
        staged = c->up_buf[slot];
        a.src = c->scale_src;
        a.sstride = (int)row;
    }
    const int rc = klt_run(c, [=](hipStream_t st) {
        if (staged) XR_HIP(hipMemcpyAsync(c->scale_src, staged, bytes, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_upload_scaled, grid, dim3(256), 0, st, a);
        XR_HIP(hipGetLastError());
        return XRHIP_OK;
    });
    if (rc || !staged) return rc;
    return slot_in_flight(c, slot);
}

// A Bayer mosaic (XRHIP_PIXFMT_BAYER_*), demosaiced to gray by k_upload_bayer: a launch of its own in the context's order, like the
// scaled upload and for its reason -- every row of the mosaic is read by the lanes of three plane rows, so a host frame goes through
// the pinned slot to the HBM scratch (scale_src) and the kernel reads that; a mosaic in HBM is read where it lies.  Not part of the
// shared upload launch (a group member: on the group's front-end queue, behind a pending upload, which is submitted first).
// Scaled: the crop is a Bayer frame of its own (its phase shifted by the crop's origin, neighbours mirrored at its edges: only the
// crop's bytes are read); it is demosaiced into the cw x ch gray scratch, from which k_upload_scaled takes it as a gray crop.
static int upload_bayer_into(xrhip_klt *c, const FrameSource &s, uint8_t *dst) {
    const xrh::PixelFormat pf = s.scaled ? xrh::crop_pixel_format(s.pf, *s.geo) : s.pf;
    BayerArgs a{};
    a.src = s.scaled ? xrh::crop_origin(s.pixels, s.stride, *s.geo, pf.bpp) : s.pixels;
    a.sstride = s.stride;
    a.dst = dst;
    a.w = s.scaled ? s.geo->crop_width : s.pw;
    a.h = s.scaled ? s.geo->crop_height : s.ph;
    a.bpp = pf.bpp;
    a.shift = (int)pf.shift;
    a.px = pf.px;
    a.py = pf.py;
    const size_t pixels = (size_t)a.w * a.h, row = (size_t)a.w * pf.bpp, bytes = row * a.h;
    int rc = XRHIP_OK;
    if (s.scaled) {
        rc = grow_scratch(c, c->bayer_gray, c->bayer_gray_cap, pixels);
        if (rc) return rc;
        a.dst = c->bayer_gray;
    }
    const ScaleArgs sa = scale_args(s.pw, s.ph, c->bayer_gray, a.w, 1, 0, a.w, a.h, dst);   // (scaled only)
    const bool scaled = s.scaled;
    const dim3 grid = grid_of_fours(pixels), scale_grid = grid_of_fours((size_t)s.pw * s.ph);
    const uint8_t *staged = nullptr;   // host frame: the slot that holds the mosaic
    int slot = 0;
    if (!s.on_device) {
        rc = grow_scratch(c, c->scale_src, c->scale_cap, bytes);
        if (rc) return rc;
        rc = slot_fill(c, a.src, s.stride, row, a.h, slot);
        if (rc) return rc;
        staged = c->up_buf[slot];
        a.src = c->scale_src;
        a.sstride = (int)row;
    }
    rc = klt_run(c, [=](hipStream_t st) {
        if (staged) XR_HIP(hipMemcpyAsync(c->scale_src, staged, bytes, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_upload_bayer, grid, dim3(256), 0, st, a);
        XR_HIP(hipGetLastError());
        if (scaled) {
            hipLaunchKernelGGL(k_upload_scaled, scale_grid, dim3(256), 0, st, sa);
            XR_HIP(hipGetLastError());
        }
        return XRHIP_OK;
    });
    if (rc || !staged) return rc;
    return slot_in_flight(c, slot);
}

// Packed 10 / 12-bit samples (XRHIP_PIXFMT_*_MIPI, *10P, *12P), unpacked by k_upload_packed: launches of their own in the context's
// order, like the Bayer upload (a group member: on the group's front-end queue, behind a pending upload, which is submitted first).
//   a mono frame of the plane's size   k_upload_packed -> the plane                                                    1 launch
//   a scaled mono frame                k_upload_packed -> the crop's 8-bit samples in scale_src; k_upload_scaled       2
//   a mosaic                           k_upload_packed -> its 8-bit samples in scale_src; k_upload_bayer               2
//   a scaled mosaic                    ... k_upload_bayer -> bayer_gray; k_upload_scaled                               3
// Exact: the Bayer and scaled definitions reduce a sample to 8 bits before anything else.  Only the byte groups that hold a pixel of
// the frame (scaled: of the crop) are read.  A host frame: those bytes, packed, go through the pinned slot, which the kernel reads
// mapped -- every sample is unpacked by one lane, so its bytes cross the host link once (a dword at the seam of two lanes' runs may be
// fetched by both, as in k_upload), at 1.25 / 1.5 bytes a pixel.
static int upload_packed_into(xrhip_klt *c, const FrameSource &s, uint8_t *dst) {
    const xrh::PixelFormat pf = s.scaled ? xrh::crop_pixel_format(s.pf, *s.geo) : s.pf;
    const int rw = s.scaled ? s.geo->crop_width : s.pw, rh = s.scaled ? s.geo->crop_height : s.ph;
    const xrhip_frame_geometry whole{s.pw, s.ph, 0, 0, s.pw, s.ph};
    PackedArgs a{};
    a.src = xrh::crop_rows(s.pixels, s.stride, s.scaled ? *s.geo : whole, pf, a.x0);
    a.sstride = s.stride;
    a.dst = dst;
    a.w = rw;
    a.h = rh;
    a.bits = pf.bits;
    a.mipi = pf.packing == xrh::PixelFormat::PACK_MIPI;
    a.limited = pf.limited;
    const size_t pixels = (size_t)rw * rh;
    const bool scaled = s.scaled, bayer = pf.bayer;
    int rc = XRHIP_OK;
    if (scaled || bayer) {   // the 8-bit samples, for the kernels that follow
        rc = grow_scratch(c, c->scale_src, c->scale_cap, (pixels + 3) & ~(size_t)3);
        if (rc) return rc;
        a.dst = c->scale_src;
    }
    if (scaled && bayer) {
        rc = grow_scratch(c, c->bayer_gray, c->bayer_gray_cap, pixels);
        if (rc) return rc;
    }
    BayerArgs ba{};
    ba.src = c->scale_src;
    ba.sstride = rw;
    ba.dst = scaled ? c->bayer_gray : dst;
    ba.w = rw;
    ba.h = rh;
    ba.bpp = 1;
    ba.px = pf.px;
    ba.py = pf.py;
    const ScaleArgs sa = scale_args(s.pw, s.ph, bayer ? c->bayer_gray : c->scale_src, rw, 1, 0, rw, rh, dst);   // (scaled only)
    const dim3 grid = grid_of_fours(pixels), scale_grid = grid_of_fours((size_t)s.pw * s.ph);
    int slot = -1;
    if (!s.on_device) {
        const size_t row = (size_t)pf.row_bytes((long long)a.x0 + rw);
        rc = slot_fill(c, a.src, s.stride, row, rh, slot);
        if (rc) return rc;
        uint8_t *dbuf = nullptr;
        XR_HIP(hipHostGetDevicePointer((void **)&dbuf, c->up_buf[slot], 0));
        a.src = dbuf;
        a.sstride = (int)row;
    }
    rc = klt_run(c, [=](hipStream_t st) {
        hipLaunchKernelGGL(k_upload_packed, grid, dim3(256), 0, st, a);
        XR_HIP(hipGetLastError());
        if (bayer) {
            hipLaunchKernelGGL(k_upload_bayer, grid, dim3(256), 0, st, ba);
            XR_HIP(hipGetLastError());
        }
        if (scaled) {
            hipLaunchKernelGGL(k_upload_scaled, scale_grid, dim3(256), 0, st, sa);
            XR_HIP(hipGetLastError());
        }
        return XRHIP_OK;
    });
    if (rc || slot < 0) return rc;
    return slot_in_flight(c, slot);
}

// Every xrhip_image_upload* entry point (`who`).  distorted: the frame is as the camera recorded it and k_undistort rectifies it into
// the plane -- reduced / scaled into undist_src first, rectified second: the gray frame takes the place of the one a gray camera of
// the plane's size would have recorded; such a frame already in HBM is remapped where it lies.
//
// Under an orientation (xrhip_klt_set_orientation, o != 0) the same uploads run in the source's orientation -- the plane they write is
// orient_src, h x w for odd r (s.pw x s.ph); exact area scaling commutes with the eight orientations, so the working-size result is
// what is turned -- and k_orient turns it into the plane (or undist_src) with a launch of its own in the context's order, like the
// scaled upload's (a group member: on the group's front-end queue, behind its pending upload, which is submitted first).
static int upload_frame(xrhip_image *im, const FrameSource &handed, const char *bad_format, bool distorted, const char *who) {
    FrameSource s = handed;   // (a reference: the callers' bad_format argument fills in handed.pf)
    const int o = im ? im->ctx->orient : 0;
    if (im) {
        s.pw = (o & 1) ? im->ctx->h : im->ctx->w;
        s.ph = (o & 1) ? im->ctx->w : im->ctx->h;
    }
    int rc = check_frame(who, im, s, bad_format);
    if (rc) return rc;
    xrhip_klt *c = im->ctx;
    if (distorted && !c->have_undist) return frame_fail(XRHIP_ESTATE, who, "no undistortion map (xrhip_klt_set_undistort_map)");
    const uint8_t *remap_src = c->undist_src;
    int remap_stride = c->w;
    if (o == 0 && distorted && s.on_device && !s.scaled && !s.pf.bayer && !s.pf.packing && s.pf.bpp == 1 && upf_word(s.pf) == 0) {
        remap_src = s.pixels;
        remap_stride = s.stride;
    } else {
        // (a host buffer may be reused by the caller as soon as we return: PushImage deep-copies, the pinned slot holds our copy)
        uint8_t *plane = distorted ? c->undist_src : im->raw, *dst = plane;
        if (o != 0) {
            // (once per context, by its first turned frame, like bayer_gray: hipMalloc may synchronise the device, which a group
            // member then does in the middle of the group's frame -- a one-off delay, results unchanged; the size never grows)
            if (!c->orient_src) XR_HIP(hipMalloc(&c->orient_src, ((size_t)c->w * c->h + 3) & ~(size_t)3));
            dst = c->orient_src;
        }
        rc = s.pf.packing ? upload_packed_into(c, s, dst)
             : s.pf.bayer ? upload_bayer_into(c, s, dst) : s.scaled ? upload_scaled_into(c, s, dst) : upload_into(c, s, dst);
        if (rc) return rc;
        if (o != 0) {
            // in source coordinates: r even: (fx ? w-1-X : X, fy ? h-1-Y : Y); r odd: (fx ? h-1-Y : Y, fy ? w-1-X : X)
            static const int FX[8] = {0, 0, 1, 1, 1, 1, 0, 0}, FY[8] = {0, 1, 1, 0, 0, 1, 1, 0};
            const OrientArgs a{c->orient_src, plane, c->w, c->h, o & 1, FX[o], FY[o]};
            const dim3 grid = a.transpose ? dim3((c->w + OR_T - 1) / OR_T, (c->h + OR_T - 1) / OR_T) : grid_of_fours((size_t)c->w * c->h);
            rc = klt_run(c, [=](hipStream_t st) {
                hipLaunchKernelGGL(k_orient, grid, dim3(256), 0, st, a);
                XR_HIP(hipGetLastError());
                return XRHIP_OK;
            });
            if (rc) return rc;
        }
    }
    if (distorted) {   // (not batched: a remap per frame on a path the bench's resident / rectified inputs do not take)
        rc = klt_run(c, [=](hipStream_t st) {
            hipLaunchKernelGGL(k_undistort, dim3((c->w + 63) / 64, (c->h + 3) / 4), dim3(256), 0, st, remap_src, remap_stride,
                               (const uint2 *)c->undist_map, im->raw, c->w, c->w, c->h);
            XR_HIP(hipGetLastError());
            return XRHIP_OK;
        });
        if (rc) return rc;
    }
    im->have_raw = true;
    im->have_pyramid = false;
    im->want_detect = false;
    im->detect_seq = 0;
    im->mask_on = false;   // (a per-frame mask belonged to the frame before)
    im->mask_resolved = false;
    return XRHIP_OK;
}

// ------------------------------------------------------------------------------------------------------------------ masks
// One k_mask_ingest launch in the context's order: `dst` = (src != 0) && (stat != 0), either source may be missing (not both).
// A host mask goes through the next pinned slot (packed; the caller's buffer is free on return), a mask in HBM is read where it lies.
static int ingest_mask(xrhip_klt *c, const uint8_t *src, int stride, bool on_device, const uint8_t *stat, uint8_t *dst) {
    MaskArgs a{src, stride, stat, dst, c->w, c->h};
    int slot = -1;
    if (src && !on_device) {
        const int rc = slot_fill(c, src, stride, (size_t)c->w, c->h, slot);
        if (rc) return rc;
        uint8_t *dbuf = nullptr;
        XR_HIP(hipHostGetDevicePointer((void **)&dbuf, c->up_buf[slot], 0));
        a.src = dbuf;
        a.sstride = c->w;
    }
    hipLaunchKernelGGL(k_mask_ingest, grid_of_fours((size_t)c->w * c->h), dim3(256), 0, c->stream, a);
    XR_HIP(hipGetLastError());
    return slot >= 0 ? slot_in_flight(c, slot) : XRHIP_OK;
}
static int mask_plane(const xrhip_klt *c, uint8_t *&plane) {
    if (!plane) XR_HIP(hipMalloc(&plane, ((size_t)c->w * c->h + 3) & ~(size_t)3));
    return XRHIP_OK;
}
// The frame's effective mask is decided by the first of xrhip_image_set_mask / preprocess / detect / track / xrhip_debug_get_mask after
// its upload: a frame that was handed no per-frame mask takes the static one here -- one ingest launch per masked frame either way.
// Without a static mask this is two flag tests: nothing is allocated, launched or copied.
static int resolve_mask(xrhip_image *im) {
    if (im->mask_resolved) return XRHIP_OK;
    xrhip_klt *c = im->ctx;
    if (c->static_on) {
        int rc = mask_plane(c, im->mask);
        if (rc) return rc;
        rc = ingest_mask(c, nullptr, 0, true, c->mask_static, im->mask);
        if (rc) return rc;
        im->mask_on = true;
    }
    im->mask_resolved = true;
    return XRHIP_OK;
}
static int check_mask(const char *who, const xrhip_klt *c, int stride) {
    if (c->group) return frame_fail(XRHIP_ESTATE, who, "the context is a member of a group (its shared launches are the unmasked kernels)");
    if ((long long)stride < (long long)c->w) return frame_fail(XRHIP_EINVAL, who, "stride_bytes < width");
    return XRHIP_OK;
}

int xrhip_klt_set_mask(xrhip_klt *c, const void *mask, int stride, int on_device) {
    if (!c) return xr_fail(XRHIP_EINVAL, "xrhip_klt_set_mask: null context");
    if (!mask) {   // back to "no static mask" (frames already resolved keep theirs)
        c->static_on = false;
        return XRHIP_OK;
    }
    int rc = check_mask("xrhip_klt_set_mask", c, stride);
    if (rc) return rc;
    rc = mask_plane(c, c->mask_static);
    if (rc) return rc;
    // (in the stream's order: frames resolved so far have read the plane before it changes; the caller's HBM mask is free on return)
    rc = ingest_mask(c, static_cast<const uint8_t *>(mask), stride, on_device != 0, nullptr, c->mask_static);
    if (rc) return rc;
    XR_HIP(hipStreamSynchronize(c->stream));
    c->static_on = true;
    return XRHIP_OK;
}

int xrhip_image_set_mask(xrhip_image *im, const void *mask, int stride, int on_device) {
    if (!im) return xr_fail(XRHIP_EINVAL, "xrhip_image_set_mask: img is null");
    xrhip_klt *c = im->ctx;
    if (!mask) {   // the frame is back to the static mask alone (decided at its next use)
        im->mask_on = false;
        im->mask_resolved = false;
        return XRHIP_OK;
    }
    int rc = check_mask("xrhip_image_set_mask", c, stride);
    if (rc) return rc;
    if (!im->have_raw) return xr_fail(XRHIP_ESTATE, "xrhip_image_set_mask: no image uploaded (the mask belongs to a frame)");
    rc = mask_plane(c, im->mask);
    if (rc) return rc;
    rc = ingest_mask(c, static_cast<const uint8_t *>(mask), stride, on_device != 0, c->static_on ? c->mask_static : nullptr, im->mask);
    if (rc) return rc;
    c->mask_used = true;
    im->mask_on = true;
    im->mask_resolved = true;
    return XRHIP_OK;
}

/* parity aid: the frame's effective mask, w*h bytes of 0 / 1 */
int xrhip_debug_get_mask(xrhip_image *im, uint8_t *out) {
    if (!im || !out) return xr_fail(XRHIP_EINVAL, "xrhip_debug_get_mask: null argument");
    if (!im->have_raw) return xr_fail(XRHIP_ESTATE, "xrhip_debug_get_mask: no image uploaded");
    int rc = resolve_mask(im);
    if (rc) return rc;
    if (!im->mask_on) return xr_fail(XRHIP_ESTATE, "xrhip_debug_get_mask: the image has no mask");
    xrhip_klt *c = im->ctx;
    XR_HIP(hipMemcpyAsync(out, im->mask, (size_t)c->w * c->h, hipMemcpyDeviceToHost, c->stream));
    XR_HIP(hipStreamSynchronize(c->stream));
    return XRHIP_OK;
}

int xrhip_image_upload(xrhip_image *im, const uint8_t *gray, int stride) {
    return upload_frame(im, frame_source(gray, stride, 0), nullptr, false, "xrhip_image_upload");
}
int xrhip_image_upload_device(xrhip_image *im, const void *gray_dev, int stride) {
    return upload_frame(im, frame_source(gray_dev, stride, 1), nullptr, false, "xrhip_image_upload_device");
}
int xrhip_image_upload_distorted(xrhip_image *im, const void *gray, int stride, int on_device) {
    return upload_frame(im, frame_source(gray, stride, on_device), nullptr, true, "xrhip_image_upload_distorted");
}
int xrhip_image_upload_color(xrhip_image *im, const void *pixels, int stride, int channels, int on_device) {
    FrameSource s = frame_source(pixels, stride, on_device);
    return upload_frame(im, s, describe_channels(channels, s.pf), false, "xrhip_image_upload_color");
}
int xrhip_image_upload_color_distorted(xrhip_image *im, const void *pixels, int stride, int channels, int on_device) {
    FrameSource s = frame_source(pixels, stride, on_device);
    return upload_frame(im, s, describe_channels(channels, s.pf), true, "xrhip_image_upload_color_distorted");
}
// The pixel formats (xrslam_hip.h: XRHIP_PIXFMT_*): GRAY8 without a range flag, BGR8 and BGRA8 are the older entry points' frames
int xrhip_image_upload_format(xrhip_image *im, const void *pixels, int stride, int format, int bits, int limited, int on_device) {
    FrameSource s = frame_source(pixels, stride, on_device);
    return upload_frame(im, s, xrh::describe_pixel_format(format, bits, limited, s.pf), false, "xrhip_image_upload_format");
}
int xrhip_image_upload_format_distorted(xrhip_image *im, const void *pixels, int stride, int format, int bits, int limited, int on_device) {
    FrameSource s = frame_source(pixels, stride, on_device);
    return upload_frame(im, s, xrh::describe_pixel_format(format, bits, limited, s.pf), true, "xrhip_image_upload_format_distorted");
}
int xrhip_image_upload_scaled(xrhip_image *im, const void *pixels, int stride, int format, int bits, int limited, int on_device,
                              const xrhip_frame_geometry *geo) {
    FrameSource s = frame_source(pixels, stride, on_device, geo, true);
    return upload_frame(im, s, xrh::describe_pixel_format(format, bits, limited, s.pf), false, "xrhip_image_upload_scaled");
}
int xrhip_image_upload_scaled_distorted(xrhip_image *im, const void *pixels, int stride, int format, int bits, int limited, int on_device,
                                        const xrhip_frame_geometry *geo) {
    FrameSource s = frame_source(pixels, stride, on_device, geo, true);
    return upload_frame(im, s, xrh::describe_pixel_format(format, bits, limited, s.pf), true, "xrhip_image_upload_scaled_distorted");
}

int xrhip_klt_set_orientation(xrhip_klt *c, int orientation) {
    if (!c) return xr_fail(XRHIP_EINVAL, "xrhip_klt_set_orientation: null context");
    if (orientation < 0 || orientation > 7) return xr_fail(XRHIP_EINVAL, "xrhip_klt_set_orientation: orientation must be 0..7 (quarter turns clockwise + 4 * mirrored)");
    c->orient = orientation;   // (host state read by the next upload: nothing in flight depends on it)
    return XRHIP_OK;
}
int xrhip_klt_get_orientation(const xrhip_klt *c, int *orientation) {
    if (!c || !orientation) return xr_fail(XRHIP_EINVAL, "xrhip_klt_get_orientation: null argument");
    *orientation = c->orient;
    return XRHIP_OK;
}

int xrhip_klt_set_undistort_map(xrhip_klt *c, const uint32_t *map2) {
    if (!c) return xr_fail(XRHIP_EINVAL, "xrhip_klt_set_undistort_map: null context");
    if (!map2) {   // back to "frames arrive rectified"
        c->have_undist = false;
        return XRHIP_OK;
    }
    const size_t bytes = sizeof(uint32_t) * 2 * (size_t)c->w * c->h;
    if (!c->undist_map) {
        XR_HIP(hipMalloc(&c->undist_map, bytes));
        XR_HIP(hipMalloc(&c->undist_src, (size_t)c->w * c->h));
    }
    int rc = klt_run_sync(c, [&](hipStream_t st) {
        XR_HIP(hipMemcpyAsync(c->undist_map, map2, bytes, hipMemcpyHostToDevice, st));
        return XRHIP_OK;
    });
    if (rc) return rc;
    c->have_undist = true;
    return XRHIP_OK;
}

/* parity aids: the one-launch pyramid build on / off for this context; a level's plane WITH its border (rows = h + 2 pad, the
   first `cols` = w + 2 pad columns of each padded row, pad = 21) */
int xrhip_debug_set_fused_pyramid(xrhip_klt *c, int on) {
    if (!c) return xr_fail(XRHIP_EINVAL, "xrhip_debug_set_fused_pyramid: null context");
    c->fused_pyramid = on != 0;
    return XRHIP_OK;
}
int xrhip_debug_get_level_padded(const xrhip_image *im, int level, uint8_t *out, int *rows, int *cols) {
    if (!im || level < 0 || level >= im->levels || !rows || !cols) return xr_fail(XRHIP_EINVAL, "xrhip_debug_get_level_padded: bad arguments");
    if (!im->have_pyramid) return xr_fail(XRHIP_ESTATE, "xrhip_debug_get_level_padded: preprocess() has not run");
    const LevelBuf &L = im->lv[level];
    *rows = L.h + 2 * KLT_PAD;
    *cols = L.w + 2 * KLT_PAD;
    if (!out) return XRHIP_OK;
    xrhip_klt *c = im->ctx;
    return klt_run_sync(c, [&](hipStream_t st) {
        XR_HIP(hipMemcpy2DAsync(out, (size_t)*cols, L.img - (ptrdiff_t)KLT_PAD * L.istride - KLT_PAD, L.istride, (size_t)*cols, (size_t)*rows,
                                hipMemcpyDeviceToHost, st));
        return XRHIP_OK;
    });
}

/* parity aid: the 8-bit frame preprocess() will read (after an upload / the device undistortion) */
int xrhip_debug_get_raw(xrhip_image *im, uint8_t *out) {
    if (!im || !out) return xr_fail(XRHIP_EINVAL, "xrhip_debug_get_raw: null argument");
    if (!im->have_raw) return xr_fail(XRHIP_ESTATE, "xrhip_debug_get_raw: no image uploaded");
    xrhip_klt *c = im->ctx;
    return klt_run_sync(c, [&](hipStream_t st) {
        XR_HIP(hipMemcpyAsync(out, im->raw, (size_t)c->w * c->h, hipMemcpyDeviceToHost, st));
        return XRHIP_OK;
    });
}

/* measurement aid: HIP-event time of whatever the context issues between phase 0 and phase 1 (which waits for it) */
int xrhip_debug_stream_span(xrhip_klt *c, int phase, double *ms) {
    if (!c || (phase != 0 && phase != 1)) return xr_fail(XRHIP_EINVAL, "xrhip_debug_stream_span: bad arguments");
    if (!c->span_t0) {
        XR_HIP(hipEventCreate(&c->span_t0));
        XR_HIP(hipEventCreate(&c->span_t1));
    }
    hipEvent_t e = phase ? c->span_t1 : c->span_t0;
    int rc = klt_run_sync(c, [=](hipStream_t st) {
        XR_HIP(hipEventRecord(e, st));
        return XRHIP_OK;
    });
    if (rc) return rc;
    if (phase && ms) {
        float f = 0.f;
        XR_HIP(hipEventElapsedTime(&f, c->span_t0, c->span_t1));
        *ms = f;
    }
    return XRHIP_OK;
}

int xrhip_image_preprocess(xrhip_image *im, double clip_limit, int tiles_x, int tiles_y) {
    if (!im || tiles_x < 1 || tiles_y < 1 || tiles_x * tiles_y > 4096)
        return xr_fail(XRHIP_EINVAL, "xrhip_image_preprocess: bad arguments");
    if (!im->have_raw) return xr_fail(XRHIP_ESTATE, "xrhip_image_preprocess: no image uploaded");
    xrhip_klt *c = im->ctx;
    const int w = c->w, h = c->h;
    if (w < 64 || h < 64) return xr_fail(XRHIP_EINVAL, "xrhip_image_preprocess: the tracker needs at least 64 pixels a side");
    {
        const int rc = resolve_mask(im);
        if (rc) return rc;
    }
    // cv::CLAHE extends a frame that is not a multiple of the grid in BOTH directions by tiles - size % tiles pixels: a direction
    // that divides gains a whole tile count when the other one does not (the tile kernel reflects whatever lies past the frame)
    const bool divides = w % tiles_x == 0 && h % tiles_y == 0;
    const int ew = divides ? w : w + tiles_x - w % tiles_x, eh = divides ? h : h + tiles_y - h % tiles_y;
    const int tw = ew / tiles_x, th = eh / tiles_y;
    const int tiles = tiles_x * tiles_y;
    if (tiles > c->lut_tiles) {
        hipFree(c->lut);
        c->lut = nullptr;
        XR_HIP(hipMalloc(&c->lut, (size_t)tiles * 256));
        c->lut_tiles = tiles;
    }
    const int area = tw * th;
    const float lut_scale = 255.0f / area;
    int clip = 0;
    if (clip_limit > 0.0) {
        clip = (int)(clip_limit * area / 256);
        if (clip < 1) clip = 1;
    }
    ProfScope prof(c, CAT_PRE);
    // the pyramid and its derivatives: two launches (k_pyr_a, k_pyr_b) behind the LUT kernel when every level is large enough for its
    // border to be one reflection away, else (or with the development switch) the five launches they replace
    const bool general = lk_general(c);   // any level count: the CLAHE plane, then a pyrDown and a Scharr launch per level
    bool fused = c->fused_pyramid && !general;
    for (int l = 0; l < KLT_LEVELS && fused; ++l) fused = fused && im->lv[l].w >= 2 * KLT_PAD + 2 && im->lv[l].h >= 2 * KLT_PAD + 2;
    ClaheLutArgs la{im->raw, w, w, h, tw, th, tiles_x, clip, lut_scale, c->lut, tiles};
    if (fused) {
        if (c->group) {
            int rc = group_wait_launched(&c->rq_pre);   // (its argument block is about to be rewritten)
            if (rc) return rc;
        }
        PrePayload &pp = c->a_pre;
        pp.with_upload = c->upload_pending && c->a_upload.dst == im->raw;
        if (pp.with_upload) {
            pp.up = c->a_upload;
            c->upload_pending = false;
        } else {
            int rc = flush_upload(c);
            if (rc) return rc;
        }
        pp.lut = la;
        PyrAArgs &pa = pp.pa;
        pa.raw = im->raw;
        pa.rstride = w;
        pa.tw = tw;
        pa.th = th;
        pa.tiles_x = tiles_x;
        pa.tiles_y = tiles_y;
        pa.lut = c->lut;
        pa.img0 = im->lv[0].img;
        pa.img1 = im->lv[1].img;
        pa.der0 = im->lv[0].der;
        pa.w0 = im->lv[0].w; pa.h0 = im->lv[0].h; pa.s0 = im->lv[0].istride;
        pa.w1 = im->lv[1].w; pa.h1 = im->lv[1].h; pa.s1 = im->lv[1].istride;
        pa.tiles_across = (w + PA_T - 1) / PA_T;
        pa.blocks = pa.tiles_across * ((h + PA_T - 1) / PA_T);
        PyrBArgs &pb = pp.pb;
        for (int l = 0; l < KLT_LEVELS; ++l) {
            pb.img[l] = im->lv[l].img;
            pb.der[l] = im->lv[l].der;
            pb.w[l] = im->lv[l].w;
            pb.h[l] = im->lv[l].h;
            pb.istride[l] = im->lv[l].istride;
        }
        pb.tiles_across = (pb.w[1] + PB_T - 1) / PB_T;
        pb.blocks = pb.tiles_across * ((pb.h[1] + PB_T - 1) / PB_T);
        int rc = klt_issue(c, c->rq_pre, GK_PREPROCESS, &pp, launch_preprocess_batch);
        if (rc) return rc;
        prof.finish();
        im->have_pyramid = true;
        return XRHIP_OK;
    }
    int rc = klt_run(c, [=](hipStream_t st) {   // the five-launch form (tiny images, A/B reference), un-batched
        Batch<ClaheLutArgs> bl;
        std::memset(&bl, 0, sizeof(bl));
        bl.e[0] = la;
        hipLaunchKernelGGL(k_clahe_lut, dim3(tiles, 1, 1), dim3(CL_THREADS), 0, st, bl);
        {
            const LevelBuf &L = im->lv[0];
            dim3 blk(64, 4);
            dim3 grd((w + 2 * KLT_PAD + 63) / 64, (h + 2 * KLT_PAD + 3) / 4);
            hipLaunchKernelGGL(k_clahe_apply, grd, blk, 0, st, im->raw, w, w, h, tw, th, tiles_x, tiles_y, c->lut, L.img, L.istride);
        }
        if (general) {
            const PyrViewG pg = make_view_g(im);
            for (int l = 1; l < im->levels; ++l) {
                const LevelBuf &D = im->lv[l];
                hipLaunchKernelGGL(k_pyrdown, dim3((D.w + 2 * KLT_PAD + 63) / 64, (D.h + 2 * KLT_PAD + 3) / 4), dim3(64, 4), 0, st, pg.lv[l - 1], D.img,
                                   D.w, D.h, D.istride);
            }
            for (int l = 0; l < im->levels; ++l)
                hipLaunchKernelGGL(k_scharr_level, dim3((im->lv[l].w + 63) / 64, (im->lv[l].h + 3) / 4), dim3(256), 0, st, pg.lv[l], im->lv[l].der);
            XR_HIP(hipGetLastError());
            return XRHIP_OK;
        }
        PyrView pv = make_view(im);
        for (int l = 1; l < KLT_LEVELS; ++l) {
            const LevelBuf &D = im->lv[l];
            dim3 blk(64, 4);
            dim3 grd((D.w + 2 * KLT_PAD + 63) / 64, (D.h + 2 * KLT_PAD + 3) / 4);
            hipLaunchKernelGGL(k_pyrdown, grd, blk, 0, st, pv.lv[l - 1], D.img, D.w, D.h, D.istride);
        }
        ScharrArgs sa;
        int off = 0;
        for (int l = 0; l < KLT_LEVELS; ++l) {
            sa.lv[l] = pv.lv[l];
            sa.out[l] = im->lv[l].der;
            sa.blk_off[l] = off;
            sa.blk_w[l] = (im->lv[l].w + 63) / 64;
            off += sa.blk_w[l] * ((im->lv[l].h + 3) / 4);
        }
        sa.blk_off[KLT_LEVELS] = off;
        hipLaunchKernelGGL(k_scharr, dim3(off), dim3(256), 0, st, sa);
        XR_HIP(hipGetLastError());
        return XRHIP_OK;
    });
    if (rc) return rc;
    prof.finish();
    im->have_pyramid = true;
    return XRHIP_OK;
}

int xrhip_image_release(xrhip_image *im) {
    if (!im) return xr_fail(XRHIP_EINVAL, "xrhip_image_release: null");
    // buffers are pooled per image object; releasing only invalidates the contents
    im->have_raw = false;
    im->have_pyramid = false;
    return XRHIP_OK;
}

// The argument sets of one detection: Harris response, NMS, strongest-candidate selection; results land in the pinned top
// block / header under a fresh sequence number (one detection in flight per context)
static int fill_detect(xrhip_image *im, DetectPayload &d, int seq) {
    xrhip_klt *c = im->ctx;
    PyrView pv = make_view(im);
    const int w = c->w, h = c->h;
    double scale = (double)(1 << 2) * 3;
    scale *= 255.0;
    scale = 1.0 / scale;
    const float s2 = (float)(scale * scale);
    HarrisCand *d_top = nullptr;
    SelectHeader *d_sel = nullptr;
    XR_HIP(hipHostGetDevicePointer((void **)&d_top, c->h_top, 0));
    XR_HIP(hipHostGetDevicePointer((void **)&d_sel, c->h_sel, 0));
    const int gx = (w + 63) / 64, gy = (h + 15) / 16;
    d.hr = HarrisArgs{pv.lv[0], 0.04, s2, c->resp, c->max_key, gx, gy};
    d.nms = HarrisNmsArgs{c->resp, w, h, c->max_key, 1.0e-3, c->cand, c->cand_count, c->cand_cap, gx, gy, c->sel_hist};
    // the strongest candidates the spacing pass is handed: >= 896 (150 corners visit ~400), 8 per corner asked for beyond that
    const int keep = std::min(c->top_cap - 1024, std::max(SEL_K, c->max_points > 150 ? 8 * c->max_points : SEL_K));
    d.sel = HarrisSelectArgs{c->cand, c->cand_count, c->cand_cap, c->max_key, 1.0e-3, d_top, c->top_cap, d_sel, seq, keep, c->sel_hist};
    d.mask = nullptr;
    return XRHIP_OK;
}

// a detection of its own (no tracking launch to ride behind): asynchronous
static int launch_detect(xrhip_image *im) {
    xrhip_klt *c = im->ctx;
    ProfScope prof(c, CAT_DETECT);
    if (c->group) {
        int rc = group_wait_launched(&c->rq_detect);
        if (rc) return rc;
    }
    const int seq = ++c->sel_seq;
    int rc = fill_detect(im, c->a_detect, seq);
    if (rc) return rc;
    c->a_detect.mask = im->mask_on ? im->mask : nullptr;
    rc = klt_issue(c, c->rq_detect, GK_DETECT, &c->a_detect, launch_detect_batch);
    if (rc) return rc;
    prof.finish();
    im->detect_seq = seq;
    return XRHIP_OK;
}

int xrhip_image_prefetch_detect(xrhip_image *im) {
    if (!im) return xr_fail(XRHIP_EINVAL, "xrhip_image_prefetch_detect: null image");
    im->want_detect = true;
    return XRHIP_OK;
}

int xrhip_image_detect(xrhip_image *im, const double *existing_xy, int n_exist, int max_points, double min_distance,
                       double *out_xy, int *n_out) {
    if (!im || !out_xy || !n_out || n_exist < 0 || (n_exist > 0 && !existing_xy))
        return xr_fail(XRHIP_EINVAL, "xrhip_image_detect: bad arguments");
    if (!im->have_pyramid) return xr_fail(XRHIP_ESTATE, "xrhip_image_detect: preprocess() has not run");
    xrhip_klt *c = im->ctx;
    const int w = c->w, h = c->h;
    HostProfScope hp_all(0, "detect: whole call");
    std::optional<HostProfScope> hp_gpu(std::in_place, 1, "detect: launch+D2H waits");
    bool own_launch = false;
    if (!im->detect_seq) {
        int rc = resolve_mask(im);
        if (rc) return rc;
        rc = launch_detect(im);
        if (rc) return rc;
        own_launch = true;
    }
    const int seq = im->detect_seq;
    im->detect_seq = 0;
    im->want_detect = false;
    {   // (a detection that rode behind a tracking launch: that request has been waited for by xrhip_image_track)
        GroupRequest *rq = c->group ? (own_launch ? &c->rq_detect : &c->rq_track) : nullptr;
        int rc = wait_flag(&c->h_sel->seq, seq, klt_stream(c), rq, "xrhip_image_detect", c->group ? group_side_stream(c->group, GQ_KLT) : nullptr);
        if (rc) return rc;
        c->uploads_unsynced = 0;
    }
    const int nc = c->h_sel->n_candidates, n_top = c->h_sel->n_top;
    if (nc > c->cand_cap) return xr_fail(XRHIP_EOVERFLOW, "xrhip_image_detect: corner candidate buffer overflow");
    hp_gpu.reset();
    HostProfScope hp_sel(2, "detect: host selection");
    // total order: response desc, then linear index desc (cv greaterThanPtr).  The greedy spacing pass usually
    // stops after a few hundred candidates (max_points corners), so the order is produced lazily from a heap.
    auto before = [](const HarrisCand &a, const HarrisCand &b) {   // a is visited before b
        if (a.v > b.v) return true;
        if (a.v < b.v) return false;
        return a.idx > b.idx;
    };
    auto heap_less = [&](const HarrisCand &a, const HarrisCand &b) { return before(b, a); };
    // GFTTDetector(max_points, 1e-3, 20, 3, harris) -- minDistance is the literal 20 of opencv_image.cpp:186
    auto select_from = [&](HarrisCand *hb, HarrisCand *he) {
        std::make_heap(hb, he, heap_less);
        return greedy_min_distance(
            [&](int &idx) {
                if (hb == he) return false;
                std::pop_heap(hb, he, heap_less);
                --he;
                idx = he->idx;
                return true;
            },
            w, h, 20.0, max_points);
    };
    std::vector<int> corners;
    bool need_all = n_top > c->top_cap;
    if (!need_all) {
        if (c->h_sel->sorted) {   // already in visiting order: walk it
            const HarrisCand *it = c->h_top, *end = c->h_top + n_top;
            corners = greedy_min_distance(
                [&](int &idx) {
                    if (it == end) return false;
                    idx = (it++)->idx;
                    return true;
                },
                w, h, 20.0, max_points);
        } else {
            corners = select_from(c->h_top, c->h_top + n_top);
        }
        // the pass ran out of strong candidates before it had max_points corners: the weaker ones matter after all
        need_all = n_top < nc && (max_points <= 0 || (int)corners.size() < max_points);
    }
    if (need_all) {
        HostProfScope hp_fb(12, "detect: full candidate list fallback");
        c->stats.detect_full_list += 1;
        int rc = klt_run_sync(c, [&](hipStream_t st) {
            XR_HIP(hipMemcpyAsync(c->h_cand, c->cand, sizeof(HarrisCand) * (size_t)nc, hipMemcpyDeviceToHost, st));
            return XRHIP_OK;
        });
        if (rc) return rc;
        corners = select_from(c->h_cand, c->h_cand + nc);
    }
    int n = 0;
    HostProfScope hp_po(16, "detect: poisson");
    if (!corners.empty()) {
        PoissonDisk2 filter(min_distance, w, h);
        for (int i = 0; i < n_exist; ++i) filter.preset(existing_xy[2 * i], existing_xy[2 * i + 1]);
        for (int idx : corners) {
            const double x = (double)(float)(idx % w), y = (double)(float)(idx / w);
            if (!filter.insert(x, y)) continue;
            if (x < 20 || y < 20 || x >= w - 20 || y >= h - 20) continue;
            out_xy[2 * n] = x;
            out_xy[2 * n + 1] = y;
            ++n;
        }
    }
    *n_out = n;
    return XRHIP_OK;
}

int xrhip_image_track(const xrhip_image *cur, const xrhip_image *next, const double *curr_xy, double *next_xy_inout,
                      int has_guess, uint8_t *status, int n) {
    if (!cur || !next || n < 0 || (n > 0 && (!curr_xy || !next_xy_inout || !status)))
        return xr_fail(XRHIP_EINVAL, "xrhip_image_track: bad arguments");
    if (cur->ctx != next->ctx) return xr_fail(XRHIP_EINVAL, "xrhip_image_track: images belong to different contexts");
    if (!cur->have_pyramid || !next->have_pyramid)
        return xr_fail(XRHIP_ESTATE, "xrhip_image_track: preprocess() has not run on both images");
    if (n == 0) return XRHIP_OK;
    HostProfScope hp_trk(3, "track: whole call");
    xrhip_klt *c = cur->ctx;
    int rc = resolve_mask(const_cast<xrhip_image *>(next));
    if (rc) return rc;
    // `next` has an effective mask: the LK kernel runs without its completion mailbox and k_mask_gate, behind it, gates the status
    // bytes and publishes the sequence number (cur's mask plays no part)
    const uint8_t *const gate = next->mask_on ? next->mask : nullptr;
    rc = ensure_points(c, n);
    if (rc) return rc;
    if (n > c->h_pts_cap) {
        if (c->h_pts) hipHostFree(c->h_pts);
        c->h_pts = nullptr;
        const int cap = std::max(n, std::max(512, 2 * c->h_pts_cap));
        XR_HIP(hipHostMalloc(&c->h_pts, (size_t)cap * (2 * sizeof(double2) + 1) + 64, hipHostMallocDefault));
        c->h_pts_cap = cap;
    }
    double2 *h_curr = (double2 *)c->h_pts, *h_next = h_curr + c->h_pts_cap;
    uint8_t *h_status = (uint8_t *)(h_next + c->h_pts_cap);
    std::memcpy(h_curr, curr_xy, sizeof(double2) * n);
    if (has_guess) std::memcpy(h_next, next_xy_inout, sizeof(double2) * n);
    char *d_pts = nullptr;
    int *d_seq = nullptr;
    XR_HIP(hipHostGetDevicePointer((void **)&d_pts, c->h_pts, 0));
    XR_HIP(hipHostGetDevicePointer((void **)&d_seq, c->h_trk_seq, 0));
    double2 *dv_curr = (double2 *)d_pts, *dv_next = dv_curr + c->h_pts_cap;
    uint8_t *dv_status = (uint8_t *)(dv_next + c->h_pts_cap);
    rc = flush_upload(c);
    if (rc) return rc;
    if (c->group) {
        rc = group_wait_launched(&c->rq_track);   // (its argument block is about to be rewritten)
        if (rc) return rc;
    }
    ProfScope prof(c, CAT_TRACK);
    const int seq = ++c->trk_seq;
    if (!gate) c->done_base += (unsigned)n;   // (the device counter moves only where the LK kernel counts its points done)
    unsigned *const d_done = gate ? (unsigned *)nullptr : c->d_done;
    TrackPayload &tp = c->a_track;
    tp.lk = LkTrackArgs{make_view(cur), make_view(next), dv_curr, dv_next, has_guess ? 1 : 0, dv_status, n,
                        c->profiling ? c->d_counters : (LkCounters *)nullptr, d_done, c->done_base, d_seq, seq};
    static const bool no_inline = std::getenv("XRHIP_LK_NO_INLINE") != nullptr;   // development switch (A/B)
    tp.n_inline = 0;
    if (!no_inline && n <= LK_INLINE) {
        for (int i = 0; i < n; ++i) {
            const float cx = (float)curr_xy[2 * i], cy = (float)curr_xy[2 * i + 1];   // the kernel's own double -> float conversions
            tp.inl.p[i] = has_guess ? make_float4(cx, cy, (float)next_xy_inout[2 * i], (float)next_xy_inout[2 * i + 1]) : make_float4(cx, cy, cx, cy);
        }
        tp.n_inline = n;
    }
    // the Harris pass of `next` does not depend on the tracking result: it rides right behind the tracking launch so that it runs
    // while the host digests the tracks (the wait below is on the tracking kernel's own mailbox, not on the stream)
    tp.detect = next->want_detect && !next->detect_seq;
    int det_seq = 0;
    if (tp.detect) {
        det_seq = ++c->sel_seq;
        rc = fill_detect(const_cast<xrhip_image *>(next), tp.det, det_seq);
        if (rc) return rc;
        tp.det.mask = gate;   // (the effective mask of `next`, staged since its upload)
    }
    if (c->group) {
        rc = klt_issue(c, c->rq_track, GK_TRACK, &tp, launch_track_batch);
        if (rc) return rc;
        prof.finish();
        if (tp.detect) c->stats.n_detect++;
    } else {   // launched here: the two halves keep their own event pairs (bench.py's roofline_lk is the LK kernel alone)
        const bool with_detect = tp.detect;
        tp.detect = false;
        if (lk_general(c)) {   // (never a member of a group) the kernel with runtime parameters; what follows the launch is unchanged
            const LkTrackGArgs ga{make_view_g(cur), make_view_g(next), lk_device_params(c), dv_curr, dv_next, has_guess ? 1 : 0, dv_status, n,
                                  tp.lk.counters, d_done, c->done_base, d_seq, seq};
            hipLaunchKernelGGL(k_lk_track_g, dim3(n), dim3(LK_THREADS), 0, c->stream, ga);
            XR_HIP(hipGetLastError());
        } else {
            rc = klt_issue(c, c->rq_track, GK_TRACK, &tp, launch_track_batch);
        }
        if (rc) return rc;
        if (gate) {
            hipLaunchKernelGGL(k_mask_gate, dim3(1), dim3(256), 0, c->stream, gate, c->w, c->h, (const double2 *)dv_next, dv_status, n, d_seq, seq);
            XR_HIP(hipGetLastError());
        }
        prof.finish();
        if (with_detect) {
            ProfScope prof_d(c, CAT_DETECT);
            const DetectPayload *d = &tp.det;
            launch_detect_chunk(&d, 1, c->stream);
            XR_HIP(hipGetLastError());
            prof_d.finish();
        }
        tp.detect = with_detect;
    }
    c->stats.lk_points += n;
    if (tp.detect) const_cast<xrhip_image *>(next)->detect_seq = det_seq;
    rc = wait_flag(c->h_trk_seq, seq, klt_stream(c), c->group ? &c->rq_track : nullptr, "xrhip_image_track");
    if (rc) return rc;
    c->uploads_unsynced = 0;
    // results: status first, positions only where status != 0 (reference semantics)
    for (int i = 0; i < n; ++i) {
        status[i] = h_status[i];
        if (status[i]) {
            next_xy_inout[2 * i] = h_next[i].x;
            next_xy_inout[2 * i + 1] = h_next[i].y;
        }
    }
    return XRHIP_OK;
}

int xrhip_image_lk(const xrhip_image *prev, const xrhip_image *next, const float *prev_xy, float *next_xy_inout,
                   uint8_t *status, int n) {
    if (!prev || !next || n < 0 || (n > 0 && (!prev_xy || !next_xy_inout || !status)))
        return xr_fail(XRHIP_EINVAL, "xrhip_image_lk: bad arguments");
    if (!prev->have_pyramid || !next->have_pyramid) return xr_fail(XRHIP_ESTATE, "xrhip_image_lk: preprocess() has not run");
    if (n == 0) return XRHIP_OK;
    xrhip_klt *c = prev->ctx;
    int rc = ensure_points(c, n);
    if (rc) return rc;
    return klt_run_sync(c, [&](hipStream_t st) {
        XR_HIP(hipMemcpyAsync(c->d_fprev, prev_xy, sizeof(float2) * n, hipMemcpyHostToDevice, st));
        XR_HIP(hipMemcpyAsync(c->d_fnext, next_xy_inout, sizeof(float2) * n, hipMemcpyHostToDevice, st));
        if (lk_general(c)) {
            const LkPlainGArgs ga{make_view_g(prev), make_view_g(next), lk_device_params(c), c->d_fprev, c->d_fnext, c->d_status, n,
                                  c->profiling ? c->d_counters : (LkCounters *)nullptr};
            hipLaunchKernelGGL(k_lk_plain_g, dim3(n), dim3(LK_THREADS), 0, st, ga);
        } else {
            PyrView A = make_view(prev), B = make_view(next);
            hipLaunchKernelGGL(k_lk_plain, dim3(n), dim3(LK_THREADS), 0, st, A, B, c->d_fprev, c->d_fnext, c->d_status, n);
        }
        XR_HIP(hipGetLastError());
        XR_HIP(hipMemcpyAsync(status, c->d_status, n, hipMemcpyDeviceToHost, st));
        XR_HIP(hipMemcpyAsync(next_xy_inout, c->d_fnext, sizeof(float2) * n, hipMemcpyDeviceToHost, st));
        return XRHIP_OK;
    });
}

int xrhip_image_level_dims(const xrhip_image *im, int level, int *w, int *h) {
    if (!im || level < 0 || level >= im->levels || !w || !h) return xr_fail(XRHIP_EINVAL, "xrhip_image_level_dims: bad arguments");
    *w = im->lv[level].w;
    *h = im->lv[level].h;
    return XRHIP_OK;
}

int xrhip_image_download_level(const xrhip_image *im, int level, uint8_t *img_out, int16_t *deriv_out) {
    if (!im || level < 0 || level >= im->levels) return xr_fail(XRHIP_EINVAL, "xrhip_image_download_level: bad arguments");
    if (!im->have_pyramid) return xr_fail(XRHIP_ESTATE, "xrhip_image_download_level: preprocess() has not run");
    const LevelBuf &L = im->lv[level];
    xrhip_klt *c = im->ctx;
    return klt_run_sync(c, [&](hipStream_t st) {
        if (img_out) XR_HIP(hipMemcpy2DAsync(img_out, L.w, L.img, L.istride, L.w, L.h, hipMemcpyDeviceToHost, st));
        if (deriv_out)
            XR_HIP(hipMemcpy2DAsync(deriv_out, (size_t)L.w * 4, L.der, (size_t)L.istride * 4, (size_t)L.w * 4, L.h, hipMemcpyDeviceToHost, st));
        return XRHIP_OK;
    });
}

int xrhip_image_download_harris(xrhip_image *im, float *resp_out) {
    if (!im || !resp_out) return xr_fail(XRHIP_EINVAL, "xrhip_image_download_harris: bad arguments");
    if (!im->have_pyramid) return xr_fail(XRHIP_ESTATE, "xrhip_image_download_harris: preprocess() has not run");
    xrhip_klt *c = im->ctx;
    DetectPayload d;
    int rc = fill_detect(im, d, 0);
    if (rc) return rc;
    return klt_run_sync(c, [&](hipStream_t st) {   // the response plane alone; the running maximum goes back to its reset state
        Batch<HarrisArgs> bh;
        std::memset(&bh, 0, sizeof(bh));
        bh.e[0] = d.hr;
        hipLaunchKernelGGL(k_harris, dim3(d.hr.gx, d.hr.gy, 1), dim3(256), 0, st, bh);
        XR_HIP(hipGetLastError());
        XR_HIP(hipMemcpyAsync(resp_out, c->resp, sizeof(float) * (size_t)c->w * c->h, hipMemcpyDeviceToHost, st));
        static const int init[2] = {(int)0x80000000, 0};
        XR_HIP(hipMemcpyAsync(c->max_key, init, sizeof(init), hipMemcpyHostToDevice, st));
        return XRHIP_OK;
    });
}

int xrhip_klt_set_lk_params(xrhip_klt *c, const xrhip_lk_params *p) {
    if (!c) return xr_fail(XRHIP_EINVAL, "xrhip_klt_set_lk_params: null context");
    const xrhip_lk_params def{XRHIP_KLT_WIN, XRHIP_KLT_LEVELS - 1, 30, 0.01};
    const xrhip_lk_params q = p ? *p : def;
    char msg[256];
    if (q.win < 5 || q.win > 21 || q.win % 2 == 0) {
        std::snprintf(msg, sizeof(msg), "xrhip_klt_set_lk_params: win = %d: the window is odd, 5..21", q.win);
        return xr_fail(XRHIP_EINVAL, msg);
    }
    if (q.max_level < 0 || q.max_level > KLT_MAX_LEVELS - 1) {
        std::snprintf(msg, sizeof(msg), "xrhip_klt_set_lk_params: max_level = %d: 0..%d", q.max_level, KLT_MAX_LEVELS - 1);
        return xr_fail(XRHIP_EINVAL, msg);
    }
    if (q.max_count < 1 || q.max_count > 100) {
        std::snprintf(msg, sizeof(msg), "xrhip_klt_set_lk_params: max_count = %d: 1..100", q.max_count);
        return xr_fail(XRHIP_EINVAL, msg);
    }
    if (!(q.epsilon >= 0.0 && q.epsilon <= 10.0)) {
        std::snprintf(msg, sizeof(msg), "xrhip_klt_set_lk_params: epsilon = %g: 0..10", q.epsilon);
        return xr_fail(XRHIP_EINVAL, msg);
    }
    // cv::buildOpticalFlowPyramid stops before a level that is not larger than the window; here that is an argument check.  (The
    // reference's own pair, 21 / 3, is what every context has always run, at any frame size: it stays accepted.)
    if (!(q.win == def.win && q.max_level == def.max_level)) {
        int tw = c->w, th = c->h;
        for (int l = 0; l < q.max_level; ++l) {
            tw = (tw + 1) / 2;
            th = (th + 1) / 2;
        }
        if (tw <= q.win || th <= q.win) {
            std::snprintf(msg, sizeof(msg), "xrhip_klt_set_lk_params: max_level = %d: level %d of a %d x %d frame is %d x %d, not larger than win = %d",
                          q.max_level, q.max_level, c->w, c->h, tw, th, q.win);
            return xr_fail(XRHIP_EINVAL, msg);
        }
    }
    if (c->group)
        return xr_fail(XRHIP_ESTATE, "xrhip_klt_set_lk_params: the context is a member of a group (its shared launches are the specialised kernels)");
    if (c->n_images > 0)
        return xr_fail(XRHIP_ESTATE, "xrhip_klt_set_lk_params: the context has images (their pyramid storage is sized by max_level): set the parameters first");
    c->lk = q;
    return XRHIP_OK;
}
int xrhip_klt_get_lk_params(const xrhip_klt *c, xrhip_lk_params *out) {
    if (!c || !out) return xr_fail(XRHIP_EINVAL, "xrhip_klt_get_lk_params: null argument");
    *out = c->lk;
    return XRHIP_OK;
}
int xrhip_debug_force_general_lk(xrhip_klt *c, int on) {
    if (!c) return xr_fail(XRHIP_EINVAL, "xrhip_debug_force_general_lk: null context");
    if (on && c->group) return xr_fail(XRHIP_ESTATE, "xrhip_debug_force_general_lk: the context is a member of a group");
    c->force_general = on != 0;
    return XRHIP_OK;
}

int xrhip_klt_set_profiling(xrhip_klt *c, int enable) {
    if (!c) return xr_fail(XRHIP_EINVAL, "xrhip_klt_set_profiling: null");
    c->profiling = enable != 0;
    return XRHIP_OK;
}

int xrhip_klt_get_stats(xrhip_klt *c, xrhip_klt_stats *out, int reset) {
    if (!c || !out) return xr_fail(XRHIP_EINVAL, "xrhip_klt_get_stats: null");
    int rc = resolve_pending(c);
    if (rc) return rc;
    rc = klt_run_sync(c, [&](hipStream_t st) {
        XR_HIP(hipMemcpyAsync(c->h_counters, c->d_counters, sizeof(LkCounters), hipMemcpyDeviceToHost, st));
        return XRHIP_OK;
    });
    if (rc) return rc;
    c->stats.lk_templates = (long long)c->h_counters->templates;
    c->stats.lk_iterations = (long long)c->h_counters->iterations;
    *out = c->stats;
    if (reset) {
        c->stats = xrhip_klt_stats{};
        rc = klt_run_sync(c, [&](hipStream_t st) {
            XR_HIP(hipMemsetAsync(c->d_counters, 0, sizeof(LkCounters), st));
            return XRHIP_OK;
        });
        if (rc) return rc;
    }
    return XRHIP_OK;
}

// The tracking view of a frame: segments and markers over its gray plane (include/xrslam_hip.h has the semantics).  Three steps on the
// context's OWN stream -- clear the owner plane, k_view_stamp, k_view_compose -- behind whatever the context still has queued on the
// plane: a member of a group submits a pending upload, waits for its requests on the group's queue and renders then.
int xrhip_image_render_view(xrhip_image *im, const xrhip_view_segment *segs, int n_segs, const xrhip_view_marker *markers, int n_markers,
                            const uint8_t *palette_bgr, int n_palette, void *out, int stride, int channels, int on_device) {
    if (!im || !out || (n_segs > 0 && !segs) || (n_markers > 0 && !markers) || (n_palette > 0 && !palette_bgr))
        return xr_fail(XRHIP_EINVAL, "xrhip_image_render_view: null argument");
    if (channels != 3 && channels != 4) return xr_fail(XRHIP_EINVAL, "xrhip_image_render_view: channels must be 3 (BGR) or 4 (BGRA)");
    xrhip_klt *c = im->ctx;
    if ((long long)stride < (long long)c->w * channels) return xr_fail(XRHIP_EINVAL, "xrhip_image_render_view: stride_bytes < width * channels");
    if (n_segs < 0 || n_markers < 0 || n_palette < 0 || n_palette > 256 || n_segs > VIEW_MAX_PRIMS || n_markers > VIEW_MAX_PRIMS)
        return xr_fail(XRHIP_EINVAL, "xrhip_image_render_view: bad primitive or palette count");
    auto coord_ok = [](int v) { return v >= -VIEW_COORD_MAX - 1 && v <= VIEW_COORD_MAX; };
    for (int i = 0; i < n_segs; ++i) {
        const xrhip_view_segment &s = segs[i];
        if (!coord_ok(s.x0) || !coord_ok(s.y0) || !coord_ok(s.x1) || !coord_ok(s.y1))
            return xr_fail(XRHIP_EINVAL, "xrhip_image_render_view: segment coordinate outside [-8192, 8191]");
        if (s.style >= (uint32_t)n_palette) return xr_fail(XRHIP_EINVAL, "xrhip_image_render_view: segment palette index >= n_palette");
    }
    for (int i = 0; i < n_markers; ++i) {
        const xrhip_view_marker &m = markers[i];
        if (!coord_ok(m.x) || !coord_ok(m.y)) return xr_fail(XRHIP_EINVAL, "xrhip_image_render_view: marker coordinate outside [-8192, 8191]");
        if ((m.style & 255u) >= (uint32_t)n_palette) return xr_fail(XRHIP_EINVAL, "xrhip_image_render_view: marker palette index >= n_palette");
    }
    if (!im->have_raw) return xr_fail(XRHIP_ESTATE, "xrhip_image_render_view: the image has no gray plane (released, or never uploaded)");
    static_assert(sizeof(xrhip_view_segment) == sizeof(ViewSeg) && sizeof(xrhip_view_marker) == sizeof(ViewMarker), "view primitives");
    const int w = c->w, h = c->h;
    // scratch of the view: allocated by the first render of the context
    if (!c->view_owner) {
        XR_HIP(hipMalloc(&c->view_owner, sizeof(uint32_t) * (size_t)w * h));
        XR_HIP(hipMalloc(&c->view_out, (size_t)w * h * 4));
        XR_HIP(hipEventCreateWithFlags(&c->view_done, hipEventDisableTiming));
    }
    if (c->view_busy) {   // (an HBM render still reading the staging block)
        XR_HIP(hipEventSynchronize(c->view_done));
        c->view_busy = false;
    }
    const size_t seg_bytes = sizeof(ViewSeg) * (size_t)n_segs, mk_bytes = sizeof(ViewMarker) * (size_t)n_markers;
    const size_t pal_off = (seg_bytes + mk_bytes + 15) & ~(size_t)15, need = pal_off + 768;
    if (need > c->view_stage_cap) {
        hipHostFree(c->view_stage);
        c->view_stage = nullptr;
        c->view_stage_cap = 0;
        const size_t cap = std::max(need, (size_t)16384);
        XR_HIP(hipHostMalloc(&c->view_stage, cap, hipHostMallocDefault));
        c->view_stage_cap = cap;
    }
    if (seg_bytes) std::memcpy(c->view_stage, segs, seg_bytes);
    if (mk_bytes) std::memcpy(c->view_stage + seg_bytes, markers, mk_bytes);
    std::memset(c->view_stage + pal_off, 0, 768);
    if (n_palette) std::memcpy(c->view_stage + pal_off, palette_bgr, 3 * (size_t)n_palette);
    char *dstage = nullptr;
    XR_HIP(hipHostGetDevicePointer((void **)&dstage, c->view_stage, 0));
    // everything this context has queued on the plane comes first
    int rc = flush_upload(c);
    if (rc) return rc;
    if (c->group) {
        rc = group_drain(c->group, GQ_KLT, c);
        if (rc) return rc;
        c->uploads_unsynced = 0;
    }
    hipStream_t st = c->stream;
    if (c->view_timing) {
        if (!c->view_t0) {
            XR_HIP(hipEventCreate(&c->view_t0));
            XR_HIP(hipEventCreate(&c->view_t1));
        }
        XR_HIP(hipEventRecord(c->view_t0, st));
    }
    const int prims = n_segs + n_markers;
    uint8_t *target = on_device ? static_cast<uint8_t *>(out) : c->view_out;
    const int tstride = on_device ? stride : w * channels;
    XR_HIP(hipMemsetAsync(c->view_owner, 0, sizeof(uint32_t) * (size_t)w * h, st));
    if (prims)
        hipLaunchKernelGGL(k_view_stamp, dim3((prims + 3) / 4), dim3(256), 0, st, reinterpret_cast<const ViewSeg *>(dstage), n_segs,
                           reinterpret_cast<const ViewMarker *>(dstage + seg_bytes), n_markers, c->view_owner, w, h);
    {
        const unsigned groups = (unsigned)((w + 3) / 4) * (unsigned)h;
        hipLaunchKernelGGL(k_view_compose, dim3(std::max(1u, std::min((groups + 255u) / 256u, 1024u))), dim3(256), 0, st, im->raw, c->view_owner,
                           reinterpret_cast<const uint8_t *>(dstage + pal_off), target, tstride, w, h, channels);
    }
    XR_HIP(hipGetLastError());
    if (!on_device) XR_HIP(hipMemcpy2DAsync(out, (size_t)stride, c->view_out, (size_t)tstride, (size_t)w * channels, (size_t)h, hipMemcpyDeviceToHost, st));
    if (c->view_timing) XR_HIP(hipEventRecord(c->view_t1, st));
    if (!on_device || c->group || c->view_timing) {
        // a host destination is complete on return; so is a group member's HBM destination (its later uploads travel on the group's
        // queue, which this stream does not order)
        XR_HIP(hipStreamSynchronize(st));
        if (c->view_timing) {
            float ms = 0.f;
            XR_HIP(hipEventElapsedTime(&ms, c->view_t0, c->view_t1));
            c->view_ms += ms;
            c->view_n++;
        }
    } else {
        XR_HIP(hipEventRecord(c->view_done, st));
        c->view_busy = true;
    }
    return XRHIP_OK;
}

/* measurement aid: HIP-event time of the renders of this context, first to last command (enable < 0: leave the switch alone) */
int xrhip_debug_view_timing(xrhip_klt *c, int enable, double *ms_sum, long long *n, int reset) {
    if (!c) return xr_fail(XRHIP_EINVAL, "xrhip_debug_view_timing: null");
    if (enable >= 0) c->view_timing = enable != 0;
    if (ms_sum) *ms_sum = c->view_ms;
    if (n) *n = c->view_n;
    if (reset) {
        c->view_ms = 0;
        c->view_n = 0;
    }
    return XRHIP_OK;
}

int xrhip_klt_synchronize(xrhip_klt *c) {
    if (!c) return xr_fail(XRHIP_EINVAL, "xrhip_klt_synchronize: null");
    if (c->group) return group_drain(c->group, GQ_KLT, c);
    XR_HIP(hipStreamSynchronize(c->stream));
    return XRHIP_OK;
}

}   // extern "C"

/* development aid: LK phase timers (shader cycles, summed over all points since the last reset) of -DXRHIP_KPROF builds; zeros otherwise */
extern "C" void xrhip_debug_lkprof(long long *out8, int reset) {
#ifdef XRHIP_KPROF
    unsigned long long h[8] = {0};
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(xrhip::g_lk_prof), sizeof(h)) == hipSuccess)
        for (int i = 0; i < 8; ++i) out8[i] = (long long)h[i];
    if (reset) {
        unsigned long long z[8] = {0};
        (void)hipMemcpyToSymbol(HIP_SYMBOL(xrhip::g_lk_prof), z, sizeof(z));
    }
#else
    for (int i = 0; i < 8; ++i) out8[i] = 0;
    (void)reset;
#endif
}
