// The ingest entry points, host side: ls_ted_ingest and ls_beat_ingest check the plan's tables against the recordings' lengths, so
// that no kernel index can leave a recording, stage the call (ls_staging.h) and launch the kernels of ls_ingest.hip.
#include <vector>

#include "ls_hip.h"
#include "ls_ingest.h"
#include "ls_staging.h"

namespace ls {
namespace {

// prefix sums of the recordings' lengths: where each one starts in the concatenated array
template <class T>
std::vector<int64_t> starts(const T* len, int batch, int64_t* total) {
    std::vector<int64_t> off((size_t)batch);
    int64_t at = 0;
    for (int b = 0; b < batch; ++b) { off[(size_t)b] = at; at += (int64_t)len[b]; }
    *total = at;
    return off;
}

// a window's audio lies inside its recording once reflected: 0 <= start and start + out_len <= 2 L
bool audio_windows_ok(int n_windows, int batch, const int32_t* win_clip, const int64_t* win_start, const int64_t* audio_len, int out_len) {
    for (int w = 0; w < n_windows; ++w) {
        if (win_clip[w] < 0 || win_clip[w] >= batch) return false;
        const int64_t L = audio_len[win_clip[w]];
        if (win_start[w] < 0 || win_start[w] + out_len > 2 * L) return false;
    }
    return true;
}

IngestAudio stage_audio(Staging& st, const float* audio, int64_t total, const std::vector<int64_t>& off, const int64_t* len, int batch,
                        const int64_t* win_start, int n_windows, int out_len, float* out) {
    IngestAudio au;
    au.audio = st.in(audio, (size_t)total);
    au.off = st.upload(off.data(), off.size());
    au.len = st.upload(len, (size_t)batch);
    au.win_start = st.upload(win_start, (size_t)n_windows);
    au.out_len = out_len;
    au.out = st.out(out, (size_t)n_windows * out_len);
    return au;
}

}  // namespace
}  // namespace ls

extern "C" int ls_ted_ingest(int device, const ls_ted_ingest_args* a) {
    using namespace ls;
    if (!a || !a->cfg || !a->mean_pose || !a->n_raw || !a->audio_len || !a->raw_poses || !a->audio || a->batch < 1) return LS_EINVAL;
    if (a->n_poses < 1 || a->n_poses > LS_INGEST_MAX_POSES || a->n_ext < a->n_poses || a->n_ext > LS_INGEST_MAX_EXT) return LS_EINVAL;
    if (a->n_frames < 0 || a->n_windows < 0 || a->audio_out_len < 1) return LS_EINVAL;
    if (a->n_frames && (!a->frame_offsets || !a->frame_clip || !a->frame_lo || !a->frame_hi || !a->frame_frac)) return LS_EINVAL;
    if (a->n_windows && (!a->frame_offsets || !a->win_clip || !a->win_first || !a->win_audio_start || !a->win_has_words)) return LS_EINVAL;
    const ls_post_config* c = a->cfg;
    if (c->njoints != kIngestBones || c->n_pose_joints != kIngestJoints) return LS_EINVAL;
    for (int j = 0; j < kIngestBones; ++j)
        if (c->bone_parent[j] < 0 || c->bone_parent[j] >= kIngestJoints || c->bone_child[j] < 0 || c->bone_child[j] >= kIngestJoints)
            return LS_EINVAL;
    for (int b = 0; b < a->batch; ++b)
        if (a->n_raw[b] < 1 || a->audio_len[b] < 1) return LS_EINVAL;
    if (a->n_frames || a->n_windows) {
        if (a->frame_offsets[0] != 0 || a->frame_offsets[a->batch] != a->n_frames) return LS_EINVAL;
        for (int b = 0; b < a->batch; ++b)
            if (a->frame_offsets[b + 1] < a->frame_offsets[b]) return LS_EINVAL;
    }
    for (int i = 0; i < a->n_frames; ++i) {
        const int b = a->frame_clip[i];
        if (b < 0 || b >= a->batch || i < a->frame_offsets[b] || i >= a->frame_offsets[b + 1]) return LS_EINVAL;
        if (a->frame_lo[i] < 0 || a->frame_hi[i] < 0 || a->frame_lo[i] >= a->n_raw[b] || a->frame_hi[i] >= a->n_raw[b]) return LS_EINVAL;
    }
    if (!audio_windows_ok(a->n_windows, a->batch, a->win_clip, a->win_audio_start, a->audio_len, a->audio_out_len)) return LS_EINVAL;
    for (int w = 0; w < a->n_windows; ++w) {
        const int b = a->win_clip[w];
        if (a->win_first[w] < 0 || (int64_t)a->win_first[w] + a->n_ext > a->frame_offsets[b + 1] - a->frame_offsets[b]) return LS_EINVAL;
    }
    if (hipSetDevice(device) != hipSuccess) return LS_EHIP;
    int64_t raw_total, audio_total;
    const std::vector<int64_t> raw_off = starts(a->n_raw, a->batch, &raw_total), audio_off = starts(a->audio_len, a->batch, &audio_total);
    const size_t F = (size_t)a->n_frames, W = (size_t)a->n_windows;
    Staging st(a->on_device != 0);
    IngestFrameArgs fa{};
    fa.raw = st.in(a->raw_poses, (size_t)raw_total * kIngestPose);
    fa.raw_off = st.upload(raw_off.data(), raw_off.size());
    fa.clip = st.upload(a->frame_clip, F);
    fa.lo = st.upload(a->frame_lo, F);
    fa.hi = st.upload(a->frame_hi, F);
    fa.frac = st.upload(a->frame_frac, F);
    fa.n_frames = a->n_frames;
    for (int j = 0; j < kIngestBones; ++j) { fa.bone_parent[j] = c->bone_parent[j]; fa.bone_child[j] = c->bone_child[j]; }
    fa.resampled = st.out(a->resampled, F * kIngestPose, true);
    fa.dir_vec = st.out(a->dir_vec, F * kIngestDir, true);
    TedWindowArgs wa{};
    wa.resampled = fa.resampled;
    wa.dir_vec = fa.dir_vec;
    wa.frame_off = st.upload(a->frame_offsets, (size_t)a->batch + 1);
    wa.win_clip = st.upload(a->win_clip, W);
    wa.win_first = st.upload(a->win_first, W);
    wa.win_has_words = st.upload(a->win_has_words, W);
    wa.au = stage_audio(st, a->audio, audio_total, audio_off, a->audio_len, a->batch, a->win_audio_start, a->n_windows, a->audio_out_len,
                        a->audio_out);
    for (int i = 0; i < kIngestPose; ++i) wa.mean_pose[i] = a->mean_pose[i];
    for (int i = 0; i < kIngestDir; ++i) wa.mean_dir_vec[i] = c->mean_dir_vec[i];
    wa.n_poses = a->n_poses;
    wa.n_ext = a->n_ext;
    wa.pose_seq = st.out(a->pose_seq, W * a->n_poses * kIngestPose);
    wa.vec_seq = st.out(a->vec_seq, W * a->n_poses * kIngestDir);
    wa.x = st.out(a->x, W * a->n_poses * kIngestDir);
    wa.stats = st.out(a->stats, W * LS_INGEST_N_STATS);
    wa.verdict = st.out(a->verdict, W);
    if (st.e == hipSuccess) st.chk(launch_ingest_frames(fa, 0));
    if (st.e == hipSuccess) st.chk(launch_ted_ingest_windows(wa, a->n_windows, 0));
    return st.finish();
}

extern "C" int ls_beat_ingest(int device, const ls_beat_ingest_args* a) {
    using namespace ls;
    if (!a || !a->mean_pose || !a->std_pose || !a->n_raw || !a->audio_len || !a->poses || !a->audio || a->batch < 1) return LS_EINVAL;
    if (a->n_poses < 1 || a->n_poses > 34 || a->njoints < 1 || a->njoints > 47 || a->n_windows < 0 || a->audio_out_len < 1) return LS_EINVAL;
    if (a->n_windows && (!a->win_clip || !a->win_first || !a->win_audio_start)) return LS_EINVAL;
    for (int b = 0; b < a->batch; ++b)
        if (a->n_raw[b] < 1 || a->audio_len[b] < 1) return LS_EINVAL;
    if (!audio_windows_ok(a->n_windows, a->batch, a->win_clip, a->win_audio_start, a->audio_len, a->audio_out_len)) return LS_EINVAL;
    for (int w = 0; w < a->n_windows; ++w)
        if (a->win_first[w] < 0 || (int64_t)a->win_first[w] + a->n_poses > a->n_raw[a->win_clip[w]]) return LS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return LS_EHIP;
    int64_t pose_total, audio_total;
    const std::vector<int64_t> pose_off = starts(a->n_raw, a->batch, &pose_total), audio_off = starts(a->audio_len, a->batch, &audio_total);
    const size_t W = (size_t)a->n_windows, J3 = (size_t)a->njoints * 3;
    Staging st(a->on_device != 0);
    BeatWindowArgs wa{};
    wa.poses = st.in(a->poses, (size_t)pose_total * J3);
    wa.pose_off = st.upload(pose_off.data(), pose_off.size());
    wa.win_clip = st.upload(a->win_clip, W);
    wa.win_first = st.upload(a->win_first, W);
    wa.win_has_words = a->win_has_words ? st.upload(a->win_has_words, W) : nullptr;
    wa.au = stage_audio(st, a->audio, audio_total, audio_off, a->audio_len, a->batch, a->win_audio_start, a->n_windows, a->audio_out_len,
                        a->audio_out);
    wa.mean = st.upload(a->mean_pose, J3);
    wa.std = st.upload(a->std_pose, J3);
    wa.n_poses = a->n_poses;
    wa.njoints = a->njoints;
    wa.rot6d = st.out(a->rot6d, W * a->n_poses * J3 * 2);
    wa.x = st.out(a->x, W * a->n_poses * J3 * 2);
    wa.verdict = st.out(a->verdict, W);
    if (st.e == hipSuccess) st.chk(launch_beat_ingest_windows(wa, a->n_windows, 0));
    return st.finish();
}
