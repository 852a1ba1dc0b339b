// What the ingest entry points (ls_ingest_api.cpp) hand to the kernels of ls_ingest.hip.  Every pointer is a device pointer; the
// entry has checked on the host that every table row lies inside its recording.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ls {

constexpr int kIngestJoints = 10, kIngestBones = 9;
constexpr int kIngestPose = kIngestJoints * 3, kIngestDir = kIngestBones * 3;     // floats per frame: 30 and 27

struct IngestFrameArgs {
    const float* raw;               // [sum n_raw][30]
    const int64_t* raw_off;         // [B] first raw frame of each recording
    const int32_t *clip, *lo, *hi;  // the frame table
    const float* frac;
    int n_frames;
    int bone_parent[kIngestBones], bone_child[kIngestBones];
    float* resampled;               // [n_frames][30]
    float* dir_vec;                 // [n_frames][27]
};

struct IngestAudio {
    const float* audio;             // [sum audio_len]
    const int64_t* off;             // [B] first sample of each recording
    const int64_t* len;             // [B]
    const int64_t* win_start;       // [W] first sample of the window within its recording
    int out_len;
    float* out;                     // [W][out_len] or NULL
};

struct TedWindowArgs {
    const float* resampled;
    const float* dir_vec;
    const int32_t* frame_off;       // [B] first resampled frame of each recording
    const int32_t *win_clip, *win_first;
    const unsigned char* win_has_words;
    IngestAudio au;
    float mean_pose[kIngestPose], mean_dir_vec[kIngestDir];
    int n_poses, n_ext;
    float *pose_seq, *vec_seq, *x, *stats;
    int32_t* verdict;
};

struct BeatWindowArgs {
    const float* poses;             // [sum n_raw][J * 3]
    const int64_t* pose_off;        // [B] first frame of each recording
    const int32_t *win_clip, *win_first;
    const unsigned char* win_has_words;   // may be NULL
    IngestAudio au;
    const float *mean, *std;        // [J * 3]
    int n_poses, njoints;
    float *rot6d, *x;
    int32_t* verdict;
};

hipError_t launch_ingest_frames(const IngestFrameArgs& a, hipStream_t st);
hipError_t launch_ted_ingest_windows(const TedWindowArgs& a, int n_windows, hipStream_t st);
hipError_t launch_beat_ingest_windows(const BeatWindowArgs& a, int n_windows, hipStream_t st);

}  // namespace ls
