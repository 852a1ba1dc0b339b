// The post-processing stream's handle, host side: per slot the frame count of its running series, on the device the carries, the
// per-push slot table and (for host-side pushes) the staging -- all allocated at ls_post_stream_open for `capacity` slots and
// LS_POST_STREAM_MAX_CHUNK frames, nothing grows afterwards.  A push is ls_post_stream_check, a table upload, the output memsets and
// one launch of ls_post_stream.hip on the default stream.
#include <algorithm>
#include <cstring>
#include <vector>

#include "ls_hip.h"
#include "ls_host.h"
#include "ls_post_stream.h"

using namespace ls;

struct ls_post_stream {
    int device = 0, dataset = 0, S = 0, J = 0, F = 3, order = 1;
    int joint[kPsSeries] = {};
    PostParams p{};
    std::string err;
    bool failed = false;
    std::vector<int64_t> n;               // frames of each slot's running series
    std::vector<unsigned char> table;     // host image of the slot table: int64 n [S], int32 k [S], fin [S], tile_slot [T], tile_start [T]
    DevBuf carry, d_table;
    DevBuf in, out_a, out_b, out_c, mask; // host-side pushes: frames; aligned | decoded; pose | euler; angle_diff; beat_mask
    int mask_rows() const { return dataset == 0 ? 1 : kPsSeries; }
    int mask_cap() const { return LS_POST_STREAM_MAX_CHUNK + (dataset == 0 ? 1 : LS_POST_STREAM_MAX_ORDER); }
    size_t frame_floats() const { return (size_t)J * F; }
    size_t b_floats() const { return dataset == 0 ? (size_t)p.n_pose_joints * 3 : (size_t)J * 3; }
    size_t carry_floats() const { return (size_t)S * (dataset == 0 ? frame_floats() * kPsTedCarry : (size_t)kPsBeatCarry * kPsBeatRow); }
    size_t table_bytes() const { return (size_t)S * 8 + (size_t)S * 4 * (2 + 2 * kPsSlotTiles); }
    int64_t device_bytes() const { return (int64_t)(carry.bytes + d_table.bytes + in.bytes + out_a.bytes + out_b.bytes + out_c.bytes + mask.bytes); }
};

namespace {

int allocate(ls_post_stream* h) {
    const size_t rows = (size_t)h->S * LS_POST_STREAM_MAX_CHUNK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, h->carry.ensure(h->carry_floats() * 4));
    HIPCHK(h, hipMemset(h->carry.p, 0, h->carry_floats() * 4));
    HIPCHK(h, h->d_table.ensure(h->table_bytes()));
    HIPCHK(h, h->in.ensure(rows * h->frame_floats() * 4));
    HIPCHK(h, h->out_a.ensure(rows * h->frame_floats() * 4));
    HIPCHK(h, h->out_b.ensure(rows * h->b_floats() * 4));
    if (h->dataset == 0) HIPCHK(h, h->out_c.ensure(rows * 4));
    HIPCHK(h, h->mask.ensure((size_t)h->S * h->mask_rows() * h->mask_cap()));
    return LS_OK;
}

// the launch table: units of slot s are its new frames and, for BEAT, its beat entries; returns the number of tiles
unsigned build_table(ls_post_stream* h, const int32_t* counts, const int32_t* finish, const int32_t* beat_count, PostStreamTable* dev) {
    const int S = h->S;
    unsigned char* base = h->table.data();
    int64_t* n = reinterpret_cast<int64_t*>(base);
    int32_t* k = reinterpret_cast<int32_t*>(base + (size_t)S * 8);
    int32_t *fin = k + S, *tile_slot = fin + S, *tile_start = tile_slot + (size_t)S * kPsSlotTiles;
    unsigned tiles = 0;
    for (int s = 0; s < S; ++s) {
        n[s] = h->n[(size_t)s];
        k[s] = counts[s];
        fin[s] = finish && finish[s] ? 1 : 0;
        const int units = h->dataset == 0 ? counts[s] : std::max(counts[s], beat_count[s]);
        for (int t0 = 0; t0 < units; t0 += kPsTile, ++tiles) {
            tile_slot[tiles] = s;
            tile_start[tiles] = t0;
        }
    }
    const unsigned char* d = static_cast<const unsigned char*>(h->d_table.p);
    dev->n = reinterpret_cast<const long long*>(d);
    dev->k = reinterpret_cast<const int*>(d + (size_t)S * 8);
    dev->fin = dev->k + S;
    dev->tile_slot = dev->fin + S;
    dev->tile_start = dev->tile_slot + (size_t)S * kPsSlotTiles;
    return tiles;
}

int push(ls_post_stream* h, const ls_post_stream_push_args* a, const int32_t* beat_count) {
    const int S = h->S, K = a->K, Kb = a->beat_capacity;
    const bool ted = h->dataset == 0, dev = a->on_device != 0;
    const size_t rows = (size_t)S * K, n_in = rows * h->frame_floats(), n_b = rows * h->b_floats(), n_mask = (size_t)S * h->mask_rows() * Kb;
    HIPCHK(h, hipSetDevice(h->device));
    float* out_a = ted ? a->aligned : a->decoded;
    float* out_b = ted ? a->pose : a->euler_deg;
    float* out_c = ted ? a->angle_diff : nullptr;
    const float* d_in = a->frames;
    float *d_a = out_a, *d_b = out_b, *d_c = out_c;
    unsigned char* d_mask = a->beat_mask;
    if (!dev) {                                                          // the staging of the open: K and Kb are within its bounds
        if (n_in) HIPCHK(h, hipMemcpy(h->in.p, a->frames, n_in * 4, hipMemcpyHostToDevice));
        d_in = h->in.f();
        d_a = out_a ? h->out_a.f() : nullptr;
        d_b = out_b ? h->out_b.f() : nullptr;
        d_c = out_c ? h->out_c.f() : nullptr;
        d_mask = a->beat_mask ? static_cast<unsigned char*>(h->mask.p) : nullptr;
    }
    if (d_a && n_in) HIPCHK(h, hipMemsetAsync(d_a, 0, n_in * 4, nullptr));     // rows behind a slot's count; TED's pending entry at the finish
    if (d_b && n_b) HIPCHK(h, hipMemsetAsync(d_b, 0, n_b * 4, nullptr));
    if (d_c && rows) HIPCHK(h, hipMemsetAsync(d_c, 0, rows * 4, nullptr));
    if (d_mask && n_mask) HIPCHK(h, hipMemsetAsync(d_mask, 0, n_mask, nullptr));
    PostStreamTable t{};
    const unsigned tiles = build_table(h, a->counts, a->finish, beat_count, &t);
    if (tiles) {
        HIPCHK(h, hipMemcpy(h->d_table.p, h->table.data(), h->table.size(), hipMemcpyHostToDevice));
        if (ted) {
            TedStreamArgs k{d_in, K, Kb, t, h->carry.f(), d_a, d_b, d_c, d_mask};
            HIPCHK(h, launch_ted_post_stream(h->p, k, tiles, nullptr));
        } else {
            BeatStreamArgs k{};
            k.frames = d_in; k.K = K; k.Kb = Kb; k.J = h->J; k.order = h->order; k.t = t; k.carry = h->carry.f();
            for (int s = 0; s < kPsSeries; ++s) k.joint[s] = h->joint[s];
            k.decoded = d_a; k.euler = d_b; k.beat_mask = d_mask;
            HIPCHK(h, launch_beat_post_stream(k, tiles, nullptr));
        }
    }
    HIPCHK(h, hipStreamSynchronize(nullptr));
    if (!dev) {
        if (out_a && n_in) HIPCHK(h, hipMemcpy(out_a, d_a, n_in * 4, hipMemcpyDeviceToHost));
        if (out_b && n_b) HIPCHK(h, hipMemcpy(out_b, d_b, n_b * 4, hipMemcpyDeviceToHost));
        if (out_c && rows) HIPCHK(h, hipMemcpy(out_c, d_c, rows * 4, hipMemcpyDeviceToHost));
        if (a->beat_mask && n_mask) HIPCHK(h, hipMemcpy(a->beat_mask, d_mask, n_mask, hipMemcpyDeviceToHost));
    }
    return LS_OK;
}

}  // namespace

extern "C" {

int ls_post_stream_open(int device, int32_t dataset, int32_t capacity, const ls_post_config* cfg, int32_t njoints, int32_t order,
                        const int32_t* series_joint, ls_post_stream** out) {
    using H = ls_post_stream;
    if (!out) return fail<H>(nullptr, LS_EINVAL, "ls_post_stream_open: null argument");
    if (dataset != 0 && dataset != 1) return fail<H>(nullptr, LS_EINVAL, "ls_post_stream_open: dataset %d is neither 0 (TED) nor 1 (BEAT)", dataset);
    if (capacity < 1 || capacity > (1 << 20)) return fail<H>(nullptr, LS_EINVAL, "ls_post_stream_open: capacity %d", capacity);
    PostParams p{};
    if (dataset == 0) {
        if (!post_params(cfg, &p)) return fail<H>(nullptr, LS_EINVAL, "ls_post_stream_open: bad TED configuration");
    } else {
        if (order < 1 || order > LS_POST_STREAM_MAX_ORDER)
            return fail<H>(nullptr, LS_EINVAL, "ls_post_stream_open: order %d outside [1, %d]", order, LS_POST_STREAM_MAX_ORDER);
        if (njoints < 1 || njoints > 65535 || !series_joint) return fail<H>(nullptr, LS_EINVAL, "ls_post_stream_open: njoints %d or no series joints", njoints);
        for (int s = 0; s < kPsSeries; ++s)
            if (series_joint[s] < 0 || series_joint[s] >= njoints)
                return fail<H>(nullptr, LS_EINVAL, "ls_post_stream_open: series joint %d outside [0, %d)", series_joint[s], njoints);
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail<H>(nullptr, LS_EHIP, "ls_post_stream_open: no HIP device (no CPU path exists)");
    if (device < 0 || device >= count) return fail<H>(nullptr, LS_EINVAL, "ls_post_stream_open: device %d out of range", device);
    H* h = new H();
    h->device = device; h->dataset = dataset; h->S = capacity; h->p = p;
    h->J = dataset == 0 ? p.njoints : njoints;
    h->F = dataset == 0 ? 3 : 6;
    h->order = dataset == 0 ? 1 : order;
    for (int s = 0; s < kPsSeries && dataset == 1; ++s) h->joint[s] = series_joint[s];
    h->n.assign((size_t)capacity, 0);
    h->table.assign(h->table_bytes(), 0);
    const int rc = allocate(h);
    if (rc != LS_OK) return abandon(h, ls_post_stream_close, fail<H>(nullptr, rc, "ls_post_stream_open: %s", h->err.c_str()));
    *out = h;
    return LS_OK;
}

int ls_post_stream_push(ls_post_stream* h, const ls_post_stream_push_args* a) {
    if (!h) return LS_EINVAL;
    if (!a) return fail(h, LS_EINVAL, "ls_post_stream_push: null argument");
    if (h->failed) return fail(h, LS_ESTATE, "ls_post_stream_push: an earlier push failed on the device; close the stream");
    std::vector<int64_t> first((size_t)h->S);
    std::vector<int32_t> count((size_t)h->S);
    const int rc = ls_post_stream_check(h->dataset, h->order, h->S, h->n.data(), a->K, a->counts, a->finish, a->beat_capacity, first.data(), count.data());
    if (rc != LS_OK)
        return fail(h, rc, "ls_post_stream_push: refused (counts in [0, K], K <= %d, beat_capacity >= every slot's entries, finish only on a slot with frames)",
                    LS_POST_STREAM_MAX_CHUNK);
    if (a->K > 0 && !a->frames) return fail(h, LS_EINVAL, "ls_post_stream_push: frames is NULL");
    if (a->beat_capacity > h->mask_cap()) return fail(h, LS_EINVAL, "ls_post_stream_push: beat_capacity %d above %d", a->beat_capacity, h->mask_cap());
    const int prc = push(h, a, count.data());
    if (prc != LS_OK) {
        h->failed = true;
        return prc;
    }
    for (int s = 0; s < h->S; ++s) {
        h->n[(size_t)s] = a->finish && a->finish[s] ? 0 : h->n[(size_t)s] + a->counts[s];
        if (a->beat_first) a->beat_first[s] = first[(size_t)s];
        if (a->beat_count) a->beat_count[s] = count[(size_t)s];
    }
    return LS_OK;
}

int ls_post_stream_info(const ls_post_stream* h, int64_t* frames_in, int64_t* device_bytes) {
    if (!h) return LS_EINVAL;
    if (frames_in) std::memcpy(frames_in, h->n.data(), h->n.size() * sizeof(int64_t));
    if (device_bytes) *device_bytes = h->device_bytes();
    return LS_OK;
}

void ls_post_stream_close(ls_post_stream* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    delete h;
}

const char* ls_post_stream_last_error(const ls_post_stream* h) { return last_error(h); }

}  // extern "C"
