// The resampler's entry points, host side: ls_resample (one call, the handle-less staging of ls_staging.h) and the stream's handle.
// Per slot the handle keeps the frames and outputs of its running series and which of its two carries is current; on the device the
// tap table, the carries of every slot, the per-launch slot table and the staging of host-side pushes -- all allocated at
// ls_resample_stream_open, nothing grows afterwards.  A push is the plan (ls_resample_plan.cpp) slot by slot, a table upload and two
// launches of ls_resample.hip.  Everything runs on the null stream.  The messages of ls_resample and of a failed open are this
// thread's ls_resample_stream_last_error(NULL).
#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <tuple>
#include <vector>

#include "ls_hip.h"
#include "ls_host.h"
#include "ls_resample.h"
#include "ls_staging.h"

using namespace ls;

struct ls_resample_stream {
    int device = 0, S = 0, dtype = 0, C = 1, max_chunk = 0;
    ResampleRatio q{};
    float gain = 1.f;
    long long carry_len = 0, plan_half = 0;
    std::shared_ptr<const std::vector<float>> tab;         // host image of the tap table [up, Tp] (shared with the cache below)
    std::string err;
    bool failed = false;
    std::vector<int64_t> samples, outputs;                 // per slot
    std::vector<int> parity;
    std::vector<ResampleSlotRow> rows;                     // host image of the slot table [S + 1]
    DevBuf d_tab, carry, d_rows, in_audio, out_stage;
    size_t elem() const { return dtype == LS_RESAMPLE_I16 ? 2 : 4; }
    int64_t device_bytes() const { return (int64_t)(d_tab.bytes + carry.bytes + d_rows.bytes + in_audio.bytes + out_stage.bytes); }
};

namespace {

using H = ls_resample_stream;

// The tap table of a filter, [up, Tp]: row r holds h[r + j up], j = 0 .. T - 1, zero behind the last tap.  Designing it costs an I0
// series per tap (28225 taps at 44.1 kHz), so the tables of the last few filters are kept: a one-shot call with a filter met before
// designs nothing.  Tables above 2^20 floats are not kept.
std::shared_ptr<const std::vector<float>> tap_table(int64_t up, int64_t down, int32_t zeros, double beta, double rolloff, int64_t n_taps, int Tp, int* rc) {
    using Key = std::tuple<int64_t, int64_t, int32_t, double, double>;
    static std::mutex lock;
    static std::map<Key, std::shared_ptr<const std::vector<float>>> kept;
    const Key key{up, down, zeros, beta, rolloff};
    {
        std::lock_guard<std::mutex> g(lock);
        const auto it = kept.find(key);
        if (it != kept.end()) return it->second;
    }
    std::vector<float> h((size_t)n_taps);
    *rc = ls_resample_taps(up, down, zeros, beta, rolloff, nullptr, h.data());
    if (*rc != LS_OK) return nullptr;
    auto tab = std::make_shared<std::vector<float>>((size_t)up * Tp, 0.f);
    for (int64_t r = 0; r < up; ++r)
        for (int64_t j = 0; r + j * up < n_taps; ++j) (*tab)[(size_t)(r * Tp + j)] = h[(size_t)(r + j * up)];
    if (tab->size() <= (size_t)1 << 20) {
        std::lock_guard<std::mutex> g(lock);
        if (kept.size() >= 8) kept.clear();
        kept[key] = tab;
    }
    return tab;
}

// what both forms refuse of the rates, the sample format and the filter, and what they compute from them: fills q, gain, carry_len,
// plan_half and the table of `f`
int make_filter(const char* who, int32_t in_sr, int32_t out_sr, int32_t channels, int32_t dtype, int32_t zeros, double beta, double rolloff, H* f) {
    if (dtype != LS_RESAMPLE_F32 && dtype != LS_RESAMPLE_I16) return fail<H>(nullptr, LS_EINVAL, "%s: dtype %d is neither float32 (0) nor int16 (1)", who, dtype);
    if (channels < 1 || channels > LS_RESAMPLE_MAX_CHANNELS)
        return fail<H>(nullptr, LS_EINVAL, "%s: channels %d outside [1, %d]", who, channels, LS_RESAMPLE_MAX_CHANNELS);
    if (in_sr < 1 || out_sr < 1 || zeros < 1) return fail<H>(nullptr, LS_EINVAL, "%s: in_sr %d, out_sr %d and zeros %d must be >= 1", who, in_sr, out_sr, zeros);
    if (!(beta >= 0.0) || !(rolloff > 0.0) || !(rolloff <= 1.0))
        return fail<H>(nullptr, LS_EINVAL, "%s: beta %g must be >= 0 and rolloff %g in (0, 1]", who, beta, rolloff);
    int64_t up = 0, down = 0, half = 0, T = 0, carry = 0, n_taps = 0;
    const int rc = ls_resample_ratio(in_sr, out_sr, zeros, &up, &down, &half, &T, &carry, &n_taps);
    if (rc == LS_EUNSUPPORTED)
        return fail<H>(nullptr, rc, "%s: %d -> %d Hz with %d zeros needs n_taps = %lld, above 2^22 = 4194304", who, in_sr, out_sr, zeros,
                       2LL * zeros * (std::max(in_sr, out_sr) / std::gcd(in_sr, out_sr)) + 1);
    if (rc != LS_OK) return fail<H>(nullptr, rc, "%s: ls_resample_ratio refused %d -> %d Hz, %d zeros", who, in_sr, out_sr, zeros);
    f->dtype = dtype;
    f->C = channels;
    f->gain = dtype == LS_RESAMPLE_I16 ? (float)(1.0 / (32768.0 * channels)) : (float)(1.0 / channels);
    ResampleRatio& q = f->q;
    q = ResampleRatio{};
    q.up = up; q.down = down; q.half = half;
    q.pass_through = in_sr == out_sr;
    f->plan_half = q.pass_through ? 0 : half;
    // the handle's carries hold 3 samples more than the ABI's carry_len: a row's zero padding (Tp - T <= 3 columns) then meets the same
    // samples in the stream as in the one-shot call, so the two agree bit for bit also where the input holds Inf or NaN
    f->carry_len = q.pass_through ? 1 : carry + 3;
    f->tab.reset();
    if (q.pass_through) return LS_OK;
    q.T = (int)T;
    q.Tp = (int)((T + 3) / 4 * 4);
    const long long span = ((kResampleTile - 1) * down + up - 1) / up + q.Tp;
    q.staged = span <= kResampleStage;
    q.span = q.staged ? (int)span : 0;
    q.taps_in_lds = q.staged && up * q.Tp <= kResampleTapLds;
    int trc = LS_OK;
    f->tab = tap_table(up, down, zeros, beta, rolloff, n_taps, q.Tp, &trc);
    if (!f->tab) return fail<H>(nullptr, trc, "%s: ls_resample_taps refused beta %g, rolloff %g", who, beta, rolloff);
    return LS_OK;
}

int no_device(const char* who, int device) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail<H>(nullptr, LS_EHIP, "%s: no HIP device (no CPU path exists)", who);
    if (device < 0 || device >= count) return fail<H>(nullptr, LS_EINVAL, "%s: device %d out of range", who, device);
    return LS_OK;
}

// the device half of ls_resample
int run(int device, const ls_resample_args* a, const H& f, const std::vector<long long>& lens, const std::vector<long long>& outs) {
    if (hipSetDevice(device) != hipSuccess) return fail<H>(nullptr, LS_EHIP, "ls_resample: hipSetDevice(%d) failed", device);
    const size_t B = (size_t)a->batch;
    Staging st(a->on_device != 0);
    ResampleArgs k{};
    k.q = f.q; k.dtype = f.dtype; k.C = f.C; k.gain = f.gain;
    k.row_stride = a->row_stride;
    k.audio = st.in(static_cast<const char*>(a->audio), B * (size_t)a->row_stride * f.elem());
    k.lengths = st.upload(lens.data(), B);
    k.out_lengths = st.upload(outs.data(), B);
    k.tab = f.tab ? st.upload(f.tab->data(), f.tab->size()) : nullptr;
    k.out = st.out(a->out, B * (size_t)a->out_stride);
    k.out_stride = a->out_stride;
    st.fill(k.out, 0, B * (size_t)a->out_stride * sizeof(float));
    if (st.e == hipSuccess) launch_resample(k, a->batch, *std::max_element(outs.begin(), outs.end()));
    if (st.finish() != LS_OK) return fail<H>(nullptr, LS_EHIP, "ls_resample: %s", hipGetErrorString(st.e));
    return LS_OK;
}

int allocate(H* h) {
    const size_t S = (size_t)h->S;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t tab_bytes = h->tab ? h->tab->size() * 4 : 0;
    HIPCHK(h, h->d_tab.ensure(std::max<size_t>(tab_bytes, 16)));
    if (tab_bytes) HIPCHK(h, hipMemcpy(h->d_tab.p, h->tab->data(), tab_bytes, hipMemcpyHostToDevice));
    HIPCHK(h, h->carry.ensure(S * 2 * (size_t)h->carry_len * 4));
    HIPCHK(h, hipMemset(h->carry.p, 0, S * 2 * (size_t)h->carry_len * 4));
    HIPCHK(h, h->d_rows.ensure((S + 1) * sizeof(ResampleSlotRow)));
    HIPCHK(h, h->in_audio.ensure(S * (size_t)h->max_chunk * h->C * h->elem()));
    // what one push can emit per slot: the finish of max_chunk frames on top of what was pending
    const long long most = ((long long)h->max_chunk * h->q.up + h->q.down - 1) / h->q.down + (h->plan_half + h->q.down) / h->q.down + 2;
    HIPCHK(h, h->out_stage.ensure(S * (size_t)most * 4));
    return LS_OK;
}

int push(H* h, const ls_resample_stream_push_args* a, int total_tiles, bool any_fresh, long long max_count) {
    const size_t S = (size_t)h->S;
    const bool dev = a->on_device != 0;
    HIPCHK(h, hipSetDevice(h->device));
    const void* chunk = a->audio;
    if (!dev && any_fresh) {
        HIPCHK(h, hipMemcpy(h->in_audio.p, a->audio, S * (size_t)a->n_max * h->C * h->elem(), hipMemcpyHostToDevice));
        chunk = h->in_audio.p;
    }
    HIPCHK(h, hipMemcpy(h->d_rows.p, h->rows.data(), h->rows.size() * sizeof(ResampleSlotRow), hipMemcpyHostToDevice));
    ResampleStreamArgs k{};
    k.q = h->q; k.dtype = h->dtype; k.C = h->C; k.S = h->S; k.n_max = a->n_max; k.gain = h->gain;
    k.rows = static_cast<const ResampleSlotRow*>(h->d_rows.p);
    k.chunk = chunk;
    k.carry = h->carry.f();
    k.carry_len = h->carry_len;
    k.tab = h->d_tab.f();
    // host outputs: slot s's row of the staging, at a stride of this push's largest count
    k.out = dev ? a->out : h->out_stage.f();
    k.out_capacity = dev ? a->out_capacity : max_count;
    launch_resample_stream(k, total_tiles);
    if (any_fresh) launch_resample_carry(k);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(nullptr));
    if (!dev && total_tiles)
        for (size_t s = 0; s < S; ++s)
            if (h->rows[s].out_count)
                HIPCHK(h, hipMemcpy(a->out + s * (size_t)a->out_capacity, h->out_stage.f() + s * (size_t)max_count, (size_t)h->rows[s].out_count * 4,
                                    hipMemcpyDeviceToHost));
    return LS_OK;
}

}  // namespace

extern "C" {

int ls_resample(int device, const ls_resample_args* a) {
    if (!a || !a->audio || !a->lengths || !a->out) return fail<H>(nullptr, LS_EINVAL, "ls_resample: null argument");
    if (a->batch < 1 || a->batch > 65535) return fail<H>(nullptr, LS_EINVAL, "ls_resample: batch %d outside [1, 65535]", a->batch);
    H f;
    const int rc = make_filter("ls_resample", a->in_sr, a->out_sr, a->channels, a->dtype, a->zeros, a->beta, a->rolloff, &f);
    if (rc != LS_OK) return rc;
    if (a->row_stride < 1 || a->out_stride < 1) return fail<H>(nullptr, LS_EINVAL, "ls_resample: row_stride %lld and out_stride %lld must be >= 1",
                                                               (long long)a->row_stride, (long long)a->out_stride);
    std::vector<long long> lens((size_t)a->batch), outs((size_t)a->batch);
    for (int b = 0; b < a->batch; ++b) {
        const int64_t n = a->lengths[b];
        if (n < 1 || n > 0x7fffffffLL || n > a->row_stride / a->channels)
            return fail<H>(nullptr, LS_EINVAL, "ls_resample: lengths[%d] = %lld outside [1, min(2^31 - 1, row_stride / channels = %lld)]", b, (long long)n,
                           (long long)(a->row_stride / a->channels));
        int64_t first = 0, count = 0;
        if (ls_resample_plan(f.q.up, f.q.down, f.plan_half, 0, n, 1, &first, &count) != LS_OK)
            return fail<H>(nullptr, LS_EINVAL, "ls_resample: no plan for clip %d of %lld frames", b, (long long)n);
        if (count > a->out_stride)
            return fail<H>(nullptr, LS_EINVAL, "ls_resample: clip %d has %lld outputs, out_stride is %lld", b, (long long)count, (long long)a->out_stride);
        lens[(size_t)b] = n;
        outs[(size_t)b] = count;
    }
    if (a->out_lengths)
        for (int b = 0; b < a->batch; ++b) a->out_lengths[b] = outs[(size_t)b];
    const int drc = no_device("ls_resample", device);
    if (drc != LS_OK) return drc;
    return run(device, a, f, lens, outs);
}

int ls_resample_stream_open(int device, int32_t capacity, int32_t in_sr, int32_t out_sr, int32_t channels, int32_t dtype, int32_t zeros,
                            double beta, double rolloff, int32_t max_chunk, ls_resample_stream** out) {
    if (!out) return fail<H>(nullptr, LS_EINVAL, "ls_resample_stream_open: null argument");
    if (capacity < 1 || capacity > (1 << 20)) return fail<H>(nullptr, LS_EINVAL, "ls_resample_stream_open: capacity %d outside [1, 2^20]", capacity);
    if (max_chunk < 1 || max_chunk > (1 << 28)) return fail<H>(nullptr, LS_EINVAL, "ls_resample_stream_open: max_chunk %d outside [1, 2^28]", max_chunk);
    H* h = new H();
    int rc = make_filter("ls_resample_stream_open", in_sr, out_sr, channels, dtype, zeros, beta, rolloff, h);
    if (rc == LS_OK) rc = no_device("ls_resample_stream_open", device);
    if (rc != LS_OK) {
        delete h;
        return rc;
    }
    h->device = device; h->S = capacity; h->max_chunk = max_chunk;
    h->samples.assign((size_t)capacity, 0);
    h->outputs.assign((size_t)capacity, 0);
    h->parity.assign((size_t)capacity, 0);
    h->rows.assign((size_t)capacity + 1, ResampleSlotRow{});
    rc = allocate(h);
    if (rc != LS_OK) return abandon(h, ls_resample_stream_close, fail<H>(nullptr, rc, "ls_resample_stream_open: %s", h->err.c_str()));
    *out = h;
    return LS_OK;
}

int ls_resample_stream_push(ls_resample_stream* h, const ls_resample_stream_push_args* a) {
    if (!h) return LS_EINVAL;
    if (!a || !a->lengths) return fail(h, LS_EINVAL, "ls_resample_stream_push: null argument");
    if (h->failed) return fail(h, LS_ESTATE, "ls_resample_stream_push: an earlier call failed on the device; close the stream");
    const int S = h->S;
    if (a->n_max < 0 || a->n_max > h->max_chunk) return fail(h, LS_EINVAL, "ls_resample_stream_push: n_max %d outside [0, %d]", a->n_max, h->max_chunk);
    std::vector<ResampleSlotRow> rows((size_t)S + 1, ResampleSlotRow{});
    long long tiles = 0, max_count = 0;
    bool any_fresh = false;
    for (int s = 0; s < S; ++s) {
        const int32_t n = a->lengths[s];
        const bool fin = a->finish && a->finish[s];
        if (n < 0 || n > a->n_max) return fail(h, LS_EINVAL, "ls_resample_stream_push: lengths[%d] = %d outside [0, %d]", s, n, a->n_max);
        ResampleSlotRow& r = rows[(size_t)s];
        const int64_t before = h->samples[(size_t)s];
        int64_t first = 0, count = 0;
        if (!fin && n == 0) {                              // nothing for this slot: an empty row
            first = h->outputs[(size_t)s];
        } else if (ls_resample_plan(h->q.up, h->q.down, h->plan_half, before, n, fin, &first, &count) != LS_OK) {
            return fail(h, LS_EINVAL, "ls_resample_stream_push: no plan for slot %d with %lld + %d frames (finish %d): a series that is finished must hold a sample",
                        s, (long long)before, n, (int)fin);
        }
        if (count > a->out_capacity) return fail(h, LS_EINVAL, "ls_resample_stream_push: slot %d emits %lld outputs, out_capacity is %lld", s, (long long)count,
                                                 (long long)a->out_capacity);
        r.tile_off = (int)tiles;
        r.fresh = n;
        r.parity = h->parity[(size_t)s];
        r.out_first = first;
        r.out_count = count;
        r.before = before;
        r.carry_first = std::max<int64_t>(0, before - h->carry_len);
        r.total = before + n;
        r.next_first = std::max<int64_t>(0, r.total - h->carry_len);
        tiles += (count + kResampleTile - 1) / kResampleTile;
        max_count = std::max<long long>(max_count, count);
        any_fresh = any_fresh || n > 0;
    }
    if (tiles > 0x7fffffffLL) return fail(h, LS_EINVAL, "ls_resample_stream_push: %lld tiles in one push", tiles);
    rows[(size_t)S].tile_off = (int)tiles;
    if (any_fresh && !a->audio) return fail(h, LS_EINVAL, "ls_resample_stream_push: lengths without audio");
    if (tiles && !a->out) return fail(h, LS_EINVAL, "ls_resample_stream_push: outputs without out");
    for (int s = 0; s < S; ++s) {
        if (a->out_first) a->out_first[s] = rows[(size_t)s].out_first;
        if (a->out_count) a->out_count[s] = rows[(size_t)s].out_count;
    }
    h->rows = rows;
    if (tiles || any_fresh) {
        const int rc = push(h, a, (int)tiles, any_fresh, max_count);
        if (rc != LS_OK) {
            h->failed = true;
            return rc;
        }
    }
    for (int s = 0; s < S; ++s) {
        const ResampleSlotRow& r = rows[(size_t)s];
        if (a->finish && a->finish[s]) {                   // the slot is empty again: no samples in, no carry
            h->samples[(size_t)s] = h->outputs[(size_t)s] = 0;
            if (r.fresh) h->parity[(size_t)s] ^= 1;
            continue;
        }
        if (r.fresh) h->parity[(size_t)s] ^= 1;            // k_resample_carry's rule
        h->samples[(size_t)s] = r.total;
        h->outputs[(size_t)s] = r.out_first + r.out_count;
    }
    return LS_OK;
}

int ls_resample_stream_reset(ls_resample_stream* h, int32_t slot) {
    if (!h) return LS_EINVAL;
    if (slot < 0 || slot >= h->S) return fail(h, LS_EINVAL, "ls_resample_stream_reset: slot %d outside [0, %d)", slot, h->S);
    h->samples[(size_t)slot] = h->outputs[(size_t)slot] = 0;       // with no samples in, no output reads the carry
    return LS_OK;
}

int ls_resample_stream_info(const ls_resample_stream* h, int64_t* samples_in, int64_t* outputs_done, int64_t* device_bytes) {
    if (!h) return LS_EINVAL;
    if (samples_in) std::memcpy(samples_in, h->samples.data(), h->samples.size() * sizeof(int64_t));
    if (outputs_done) std::memcpy(outputs_done, h->outputs.data(), h->outputs.size() * sizeof(int64_t));
    if (device_bytes) *device_bytes = h->device_bytes();
    return LS_OK;
}

void ls_resample_stream_close(ls_resample_stream* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    delete h;
}

const char* ls_resample_stream_last_error(const ls_resample_stream* h) { return last_error(h); }

}  // extern "C"
