// The score stream's handle, host side.  Per slot: the samples, decided audio frames and motion-beat entries of its running series
// and which of its two carries is current; on the device mel_db, rms, the beat bytes and the carries of every slot, the onset tables,
// the per-launch slot table, the staging of host-side pushes and ONE slot's workspace for the finish (slots finish one after the
// other) -- all allocated at ls_score_stream_open, nothing grows afterwards.  A push is the plan (ls_score_plan.cpp) slot by slot,
// a table upload and three launches of ls_score_stream.hip; a finish is the spectrum of the remaining frames, then per slot the
// tiled pick of ls_onsets_long.hip, the alignment sum and the copies out.  Everything runs on the null stream.
#include <algorithm>
#include <cstring>
#include <vector>

#include "ls_hip.h"
#include "ls_host.h"
#include "ls_onsets.h"
#include "ls_score_stream.h"

using namespace ls;

namespace {
constexpr int kScoreTile = LS_SCORE_TILE, kMelBins = 128, kFft = 2048, kFrameHop = 512;
constexpr long long kMaxAudioFrames = (1LL << 22) - 3;         // 1 + (2^31 - 2048) / 512
}  // namespace

struct ls_score_stream {
    int device = 0, dataset = 0, S = 0;
    long long maxF = 0, maxB = 0;
    ls_score_config cfg{};
    std::string err;
    bool failed = false;
    std::vector<int64_t> samples, frames, beats_in;       // per slot
    std::vector<int> parity;
    std::vector<ScoreSlotRow> rows;                       // host image of the slot table [S + 1]
    std::vector<int> first_count;                         // host image of the beat table [S][2]
    DevBuf mel_db, rms, beats, carry, d_rows, d_first_count, tables, in_audio, in_beats;
    DevBuf ws_f, ws_i, ws_small;                          // the finish: envelope | cand, raw, bt, bt_rms, list | partials, counts, sums
    size_t tab_off[5] = {};
    int nT_max() const { return (int)((maxF + kScoreTile - 1) / kScoreTile); }
    int64_t device_bytes() const {
        return (int64_t)(mel_db.bytes + rms.bytes + beats.bytes + carry.bytes + d_rows.bytes + d_first_count.bytes + tables.bytes + in_audio.bytes +
                         in_beats.bytes + ws_f.bytes + ws_i.bytes + ws_small.bytes);
    }
};

namespace {

using H = ls_score_stream;

int allocate(H* h) {
    const size_t S = (size_t)h->S, F = (size_t)h->maxF, B = (size_t)h->maxB;
    const OnsetTables tab = make_onset_tables(h->cfg.sr, kFft, kMelBins, 0.0, h->cfg.fmax);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, h->mel_db.ensure(S * F * kMelBins * 4));
    HIPCHK(h, h->rms.ensure(S * F * 4));
    HIPCHK(h, h->beats.ensure(std::max<size_t>(S * B, 1)));
    HIPCHK(h, h->carry.ensure(S * 2 * kScoreCarry * 4));
    HIPCHK(h, hipMemset(h->carry.p, 0, S * 2 * kScoreCarry * 4));
    HIPCHK(h, h->d_rows.ensure((S + 1) * sizeof(ScoreSlotRow)));
    HIPCHK(h, h->d_first_count.ensure(S * 2 * sizeof(int)));
    HIPCHK(h, h->in_audio.ensure(S * (size_t)h->cfg.max_chunk * 4));
    HIPCHK(h, h->in_beats.ensure(S * (size_t)LS_SCORE_STREAM_MAX_BEATS));
    // the tables, one allocation: window, twiddle, mel_ptr, mel_col, mel_w (each 16-byte aligned)
    const size_t sizes[5] = {tab.window.size() * 4, tab.twiddle.size() * 4, tab.mel_ptr.size() * 4, tab.mel_col.size() * 4, tab.mel_w.size() * 4};
    const void* src[5] = {tab.window.data(), tab.twiddle.data(), tab.mel_ptr.data(), tab.mel_col.data(), tab.mel_w.data()};
    size_t total = 0;
    for (int i = 0; i < 5; ++i) {
        h->tab_off[i] = total;
        total += (sizes[i] + 15) / 16 * 16;
    }
    HIPCHK(h, h->tables.ensure(std::max<size_t>(total, 16)));
    for (int i = 0; i < 5; ++i)
        if (sizes[i]) HIPCHK(h, hipMemcpy(static_cast<char*>(h->tables.p) + h->tab_off[i], src[i], sizes[i], hipMemcpyHostToDevice));
    HIPCHK(h, h->ws_f.ensure(F * 4));
    HIPCHK(h, h->ws_i.ensure((4 * F + std::max<size_t>(B, 1)) * 4));
    HIPCHK(h, h->ws_small.ensure(((size_t)3 * h->nT_max() + 16) * 4 + 16));
    return LS_OK;
}

ScoreSpectrumArgs spectrum_args(const H* h, const float* chunk, int n_max) {
    ScoreSpectrumArgs a{};
    const char* t = static_cast<const char*>(h->tables.p);
    a.S = h->S; a.n_max = n_max; a.pad_mode = h->cfg.pad_mode; a.max_frames = h->maxF;
    a.rows = static_cast<const ScoreSlotRow*>(h->d_rows.p);
    a.chunk = chunk;
    a.carry = h->carry.f();
    a.window = reinterpret_cast<const float*>(t + h->tab_off[0]);
    a.twiddle = reinterpret_cast<const float2*>(t + h->tab_off[1]);
    a.mel_ptr = reinterpret_cast<const int*>(t + h->tab_off[2]);
    a.mel_col = reinterpret_cast<const int*>(t + h->tab_off[3]);
    a.mel_w = reinterpret_cast<const float*>(t + h->tab_off[4]);
    a.mel_db = h->mel_db.f();
    a.rms = h->rms.f();
    return a;
}

// the index in the series of the first sample a series with `frames` decided frames still needs
int64_t carry_first_of(int64_t frames) { return std::max<int64_t>(0, frames * kFrameHop - kFft / 2); }

// fills h->rows from each slot's new samples and decided frames; returns the number of new frames
int build_rows(H* h, const int32_t* fresh, const int32_t* new_frames) {
    int total = 0;
    for (int s = 0; s < h->S; ++s) {
        ScoreSlotRow& r = h->rows[(size_t)s];
        const int64_t before = h->samples[(size_t)s], done = h->frames[(size_t)s];
        r.frame_off = total;
        r.frame_first = (int)done;
        r.before = (int)before;
        r.carry_first = (int)carry_first_of(done);
        r.fresh = fresh ? fresh[s] : 0;
        r.total = (int)(before + r.fresh);
        r.parity = h->parity[(size_t)s];
        r.next_first = (int)carry_first_of(done + new_frames[s]);
        total += new_frames[s];
    }
    h->rows[(size_t)h->S] = ScoreSlotRow{};
    h->rows[(size_t)h->S].frame_off = total;
    return total;
}

int push(H* h, const ls_score_stream_push_args* a, const int32_t* fresh, const int32_t* new_frames, bool any_audio, bool any_beats) {
    const int S = h->S;
    const bool dev = a->on_device != 0;
    HIPCHK(h, hipSetDevice(h->device));
    if (any_audio) {
        const float* chunk = a->audio;
        if (!dev) {
            HIPCHK(h, hipMemcpy(h->in_audio.p, a->audio, (size_t)S * a->n_max * 4, hipMemcpyHostToDevice));
            chunk = h->in_audio.f();
        }
        const int total = build_rows(h, fresh, new_frames);
        HIPCHK(h, hipMemcpy(h->d_rows.p, h->rows.data(), h->rows.size() * sizeof(ScoreSlotRow), hipMemcpyHostToDevice));
        const ScoreSpectrumArgs k = spectrum_args(h, chunk, a->n_max);
        launch_score_spectrum(k, total);
        launch_score_carry(k);
    }
    if (any_beats) {
        const unsigned char* src = a->beats;
        if (!dev) {
            HIPCHK(h, hipMemcpy(h->in_beats.p, a->beats, (size_t)S * a->beat_capacity, hipMemcpyHostToDevice));
            src = static_cast<const unsigned char*>(h->in_beats.p);
        }
        for (int s = 0; s < S; ++s) {
            h->first_count[(size_t)2 * s] = (int)h->beats_in[(size_t)s];
            h->first_count[(size_t)2 * s + 1] = a->beat_count[s];
        }
        HIPCHK(h, hipMemcpy(h->d_first_count.p, h->first_count.data(), h->first_count.size() * sizeof(int), hipMemcpyHostToDevice));
        launch_score_beats(src, S, a->beat_capacity, static_cast<const int*>(h->d_first_count.p), static_cast<unsigned char*>(h->beats.p), h->maxB);
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(nullptr));
    return LS_OK;
}

// one finishing slot: the pick on its F frames, the alignment sum, the copies out
int finish_slot(H* h, int s, int F, const ls_score_stream_outputs* o) {
    const size_t maxF = (size_t)h->maxF, nT = (size_t)((F + kScoreTile - 1) / kScoreTile);
    int* wi = static_cast<int*>(h->ws_i.p);
    float* small = static_cast<float*>(h->ws_small.p);
    LongPickParams p{};
    p.F = F; p.nT = (int)nT; p.delta = h->cfg.delta;
    long_pick_windows(&p, (double)h->cfg.sr_pick);
    p.mel_db = h->mel_db.f() + (size_t)s * maxF * kMelBins;
    p.rms = h->rms.f() + (size_t)s * maxF;
    p.env = p.env_out = h->ws_f.f();
    p.cand = wi; p.onset_raw = wi + maxF; p.onset_bt = wi + 2 * maxF; p.onset_bt_rms = wi + 3 * maxF;
    int* list = wi + 4 * maxF;
    p.part = small;                                                       // [2, nT]
    p.ncand = reinterpret_cast<int*>(small + 2 * (size_t)h->nT_max());   // [nT]
    float* tail = small + 3 * (size_t)h->nT_max();                       // stat [3], count, n_list, n_beats, align, then the double (8-aligned)
    p.stat = tail;
    p.count = reinterpret_cast<int*>(tail + 3);
    int* n_list = reinterpret_cast<int*>(tail + 4);
    int* n_beats = reinterpret_cast<int*>(tail + 5);
    float* align = tail + 6;
    double* align_sum = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(tail + 8) + 7) / 8 * 8);
    launch_long_pick(p, 1);

    ScoreAlignArgs k{};
    k.beats = static_cast<const unsigned char*>(h->beats.p) + (size_t)s * h->maxB;
    k.n_entries = (int)h->beats_in[(size_t)s];
    k.list = list; k.n_list = n_list;
    const int* slabs[3] = {p.onset_raw, p.onset_bt, p.onset_bt_rms};
    k.onset_frames = h->dataset == 0 ? p.onset_raw : slabs[h->cfg.onset_source];
    k.onset_count = p.count;
    k.hop = h->cfg.hop; k.fps = h->cfg.fps; k.sigma = h->cfg.sigma;
    k.rate = h->dataset == 0 ? (double)h->cfg.sr : h->cfg.time_rate;
    k.align_sum = align_sum; k.n_beats = n_beats; k.align = align;
    const bool want_align = h->dataset == 0 ? (o->align_sum || o->n_beats) : o->align != nullptr;
    if (want_align) launch_score_align(k, h->dataset == 1);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(nullptr));

    const hipMemcpyKind kind = o->on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    const size_t row = (size_t)s * o->cols, n = (size_t)F * 4;
    if (o->count) HIPCHK(h, hipMemcpy(o->count + s, p.count, 4, kind));
    if (o->onset_raw) HIPCHK(h, hipMemcpy(o->onset_raw + row, p.onset_raw, n, kind));
    if (o->onset_bt) HIPCHK(h, hipMemcpy(o->onset_bt + row, p.onset_bt, n, kind));
    if (o->onset_bt_rms) HIPCHK(h, hipMemcpy(o->onset_bt_rms + row, p.onset_bt_rms, n, kind));
    if (o->oenv) HIPCHK(h, hipMemcpy(o->oenv + row, p.env, n, kind));
    if (o->rms) HIPCHK(h, hipMemcpy(o->rms + row, p.rms, n, kind));
    if (o->mel_db) HIPCHK(h, hipMemcpy(o->mel_db + row * kMelBins, p.mel_db, n * kMelBins, kind));
    if (h->dataset == 0) {
        if (o->align_sum) HIPCHK(h, hipMemcpy(o->align_sum + s, align_sum, 8, kind));
        if (o->n_beats) HIPCHK(h, hipMemcpy(o->n_beats + s, n_beats, 4, kind));
    } else if (o->align) {
        HIPCHK(h, hipMemcpy(o->align + s, align, 4, kind));
    }
    return LS_OK;
}

// counts[s]: the frames slot s still owes (0 for a slot that does not finish); marks[s] < 0: the slot does not finish
int finish(H* h, const int32_t* counts, const int32_t* marks, const ls_score_stream_outputs* o) {
    HIPCHK(h, hipSetDevice(h->device));
    const int total = build_rows(h, nullptr, counts);
    if (total) {
        HIPCHK(h, hipMemcpy(h->d_rows.p, h->rows.data(), h->rows.size() * sizeof(ScoreSlotRow), hipMemcpyHostToDevice));
        launch_score_spectrum(spectrum_args(h, nullptr, 0), total);
        HIPCHK(h, hipGetLastError());
    }
    for (int s = 0; s < h->S; ++s) {
        if (marks[s] < 0) continue;
        const int rc = finish_slot(h, s, (int)(h->frames[(size_t)s] + counts[s]), o);
        if (rc != LS_OK) return rc;
    }
    return LS_OK;
}

}  // namespace

extern "C" {

int ls_score_stream_open(int device, int32_t dataset, int32_t capacity, int32_t max_audio_frames, int32_t max_beat_entries,
                         const ls_score_config* c, ls_score_stream** out) {
    if (!out || !c) return fail<H>(nullptr, LS_EINVAL, "ls_score_stream_open: null argument");
    if (dataset != 0 && dataset != 1) return fail<H>(nullptr, LS_EINVAL, "ls_score_stream_open: dataset %d is neither 0 (TED) nor 1 (BEAT)", dataset);
    if (capacity < 1 || capacity > (1 << 20)) return fail<H>(nullptr, LS_EINVAL, "ls_score_stream_open: capacity %d", capacity);
    if (max_audio_frames < 1 || max_audio_frames > kMaxAudioFrames || max_beat_entries < 0)
        return fail<H>(nullptr, LS_EINVAL, "ls_score_stream_open: max_audio_frames %d outside [1, 2^22 - 3] or max_beat_entries %d < 0", max_audio_frames,
                       max_beat_entries);
    if (c->pad_mode != LS_ONSETS_PAD_CONSTANT && c->pad_mode != LS_ONSETS_PAD_REFLECT)
        return fail<H>(nullptr, LS_EINVAL, "ls_score_stream_open: pad_mode %d", c->pad_mode);
    if (!(c->sr > 0.f) || !(c->sr_pick > 0.f) || !(c->fmax > 0.f) || !(c->fps > 0.0) || !(c->sigma > 0.0) || !(c->time_rate > 0.0) || c->hop < 1)
        return fail<H>(nullptr, LS_EINVAL, "ls_score_stream_open: sr, sr_pick, fmax, fps, sigma and time_rate must be > 0, hop >= 1");
    if (c->onset_source < 0 || c->onset_source > 2) return fail<H>(nullptr, LS_EINVAL, "ls_score_stream_open: onset_source %d outside {0, 1, 2}", c->onset_source);
    if (c->max_chunk < 1) return fail<H>(nullptr, LS_EINVAL, "ls_score_stream_open: max_chunk %d", c->max_chunk);
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail<H>(nullptr, LS_EHIP, "ls_score_stream_open: no HIP device (no CPU path exists)");
    if (device < 0 || device >= count) return fail<H>(nullptr, LS_EINVAL, "ls_score_stream_open: device %d out of range", device);
    H* h = new H();
    h->device = device; h->dataset = dataset; h->S = capacity; h->maxF = max_audio_frames; h->maxB = max_beat_entries; h->cfg = *c;
    h->samples.assign((size_t)capacity, 0);
    h->frames.assign((size_t)capacity, 0);
    h->beats_in.assign((size_t)capacity, 0);
    h->parity.assign((size_t)capacity, 0);
    h->rows.assign((size_t)capacity + 1, ScoreSlotRow{});
    h->first_count.assign((size_t)capacity * 2, 0);
    const int rc = allocate(h);
    if (rc != LS_OK) return abandon(h, ls_score_stream_close, fail<H>(nullptr, rc, "ls_score_stream_open: %s", h->err.c_str()));
    *out = h;
    return LS_OK;
}

int ls_score_stream_push(ls_score_stream* h, const ls_score_stream_push_args* a) {
    if (!h) return LS_EINVAL;
    if (!a) return fail(h, LS_EINVAL, "ls_score_stream_push: null argument");
    if (h->failed) return fail(h, LS_ESTATE, "ls_score_stream_push: an earlier call failed on the device; close the stream");
    const int S = h->S;
    if (a->audio && (!a->lengths || a->n_max < 0 || a->n_max > h->cfg.max_chunk))
        return fail(h, LS_EINVAL, "ls_score_stream_push: audio needs lengths and n_max in [0, %d], got %d", h->cfg.max_chunk, a->n_max);
    if (a->beats && (!a->beat_first || !a->beat_count || a->beat_capacity < 0 || a->beat_capacity > LS_SCORE_STREAM_MAX_BEATS))
        return fail(h, LS_EINVAL, "ls_score_stream_push: beats need beat_first, beat_count and beat_capacity in [0, %d], got %d", LS_SCORE_STREAM_MAX_BEATS,
                    a->beat_capacity);
    std::vector<int32_t> fresh((size_t)S, 0), new_frames((size_t)S, 0);
    bool any_audio = false, any_beats = false;
    for (int s = 0; s < S; ++s) {
        if (a->audio) {
            const int32_t n = a->lengths[s];
            if (n < 0 || n > a->n_max) return fail(h, LS_EINVAL, "ls_score_stream_push: lengths[%d] = %d outside [0, %d]", s, n, a->n_max);
            int64_t first = 0;
            if (ls_score_stream_plan(h->cfg.pad_mode, h->samples[(size_t)s], n, 0, &first, &new_frames[(size_t)s]) != LS_OK)
                return fail(h, LS_EINVAL, "ls_score_stream_push: slot %d would hold more than 2^31 - 2048 samples", s);
            if (1 + (h->samples[(size_t)s] + n) / kFrameHop > h->maxF)
                return fail(h, LS_ESTATE, "ls_score_stream_push: slot %d would hold %lld audio frames, above max_audio_frames %lld", s,
                            (long long)(1 + (h->samples[(size_t)s] + n) / kFrameHop), h->maxF);
            fresh[(size_t)s] = n;
            any_audio = any_audio || n > 0;
        }
        if (a->beats) {
            const int32_t n = a->beat_count[s];
            if (n < 0 || n > a->beat_capacity) return fail(h, LS_EINVAL, "ls_score_stream_push: beat_count[%d] = %d outside [0, %d]", s, n, a->beat_capacity);
            if (n > 0 && a->beat_first[s] != h->beats_in[(size_t)s])
                return fail(h, LS_ESTATE, "ls_score_stream_push: slot %d holds %lld beat entries, the chunk starts at %lld", s, (long long)h->beats_in[(size_t)s],
                            (long long)a->beat_first[s]);
            if (h->beats_in[(size_t)s] + n > h->maxB)
                return fail(h, LS_ESTATE, "ls_score_stream_push: slot %d would hold %lld beat entries, above max_beat_entries %lld", s,
                            (long long)(h->beats_in[(size_t)s] + n), h->maxB);
            any_beats = any_beats || n > 0;
        }
    }
    if (!any_audio && !any_beats) return LS_OK;
    const int rc = push(h, a, fresh.data(), new_frames.data(), any_audio, any_beats);
    if (rc != LS_OK) {
        h->failed = true;
        return rc;
    }
    for (int s = 0; s < S; ++s) {
        if (any_audio) {
            const ScoreSlotRow& r = h->rows[(size_t)s];
            if (!(r.fresh == 0 && r.next_first == r.carry_first)) h->parity[(size_t)s] ^= 1;        // k_score_carry's rule
            h->samples[(size_t)s] += fresh[(size_t)s];
            h->frames[(size_t)s] += new_frames[(size_t)s];
        }
        if (any_beats) h->beats_in[(size_t)s] += a->beat_count[s];
    }
    return LS_OK;
}

int ls_score_stream_finish(ls_score_stream* h, const int32_t* finish_flags, const ls_score_stream_outputs* o) {
    if (!h) return LS_EINVAL;
    if (!finish_flags || !o) return fail(h, LS_EINVAL, "ls_score_stream_finish: null argument");
    if (h->failed) return fail(h, LS_ESTATE, "ls_score_stream_finish: an earlier call failed on the device; close the stream");
    const int S = h->S;
    const bool per_frame = o->onset_raw || o->onset_bt || o->onset_bt_rms || o->oenv || o->mel_db || o->rms;
    std::vector<int32_t> new_frames((size_t)S, -1);                       // -1: the slot does not finish
    bool any = false;
    for (int s = 0; s < S; ++s) {
        if (!finish_flags[s]) continue;
        const int64_t L = h->samples[(size_t)s];
        int64_t first = 0;
        if (L < 1) return fail(h, LS_ESTATE, "ls_score_stream_finish: slot %d holds no audio", s);
        if (ls_score_stream_plan(h->cfg.pad_mode, L, 0, 1, &first, &new_frames[(size_t)s]) != LS_OK)
            return fail(h, LS_ESTATE, "ls_score_stream_finish: slot %d holds %lld samples, reflect padding needs more than 1024", s, (long long)L);
        if (per_frame && 1 + L / kFrameHop > o->cols)
            return fail(h, LS_EINVAL, "ls_score_stream_finish: slot %d has %lld frames, cols is %d", s, (long long)(1 + L / kFrameHop), o->cols);
        any = true;
    }
    if (o->n_frames)
        for (int s = 0; s < S; ++s) o->n_frames[s] = new_frames[(size_t)s] < 0 ? 0 : (int32_t)(1 + h->samples[(size_t)s] / kFrameHop);
    if (!any) return LS_OK;
    std::vector<int32_t> counts((size_t)S);
    for (int s = 0; s < S; ++s) counts[(size_t)s] = std::max(new_frames[(size_t)s], 0);
    const int rc = finish(h, counts.data(), new_frames.data(), o);
    if (rc != LS_OK) {
        h->failed = true;
        return rc;
    }
    for (int s = 0; s < S; ++s)
        if (new_frames[(size_t)s] >= 0) h->samples[(size_t)s] = h->frames[(size_t)s] = h->beats_in[(size_t)s] = 0;
    return LS_OK;
}

int ls_score_stream_info(const ls_score_stream* h, int64_t* samples_in, int64_t* frames_done, int64_t* beats_in, int64_t* device_bytes) {
    if (!h) return LS_EINVAL;
    if (samples_in) std::memcpy(samples_in, h->samples.data(), h->samples.size() * sizeof(int64_t));
    if (frames_done) std::memcpy(frames_done, h->frames.data(), h->frames.size() * sizeof(int64_t));
    if (beats_in) std::memcpy(beats_in, h->beats_in.data(), h->beats_in.size() * sizeof(int64_t));
    if (device_bytes) *device_bytes = h->device_bytes();
    return LS_OK;
}

void ls_score_stream_close(ls_score_stream* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    delete h;
}

const char* ls_score_stream_last_error(const ls_score_stream* h) { return last_error(h); }

}  // extern "C"
