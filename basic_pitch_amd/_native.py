"""ctypes binding of libbasicpitch_amd.so (C ABI in include/basic_pitch_amd.h).

The product path FAILS LOUDLY when the HIP library is missing or no MI355X is visible: there is no
CPU fallback in this package (the CPU restatement under oracle/ is test infrastructure only).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from . import build as _build

BP_OK = 0
BP_ERR_INVALID_ARG = -1
BP_ERR_OUT_OF_MEMORY = -5
BP_ERR_UNSUPPORTED = -6
BP_ERR_BAD_AUDIO = -7
BP_MEM_HOST = 0
BP_MEM_DEVICE = 1
BP_FLAG_STAGE_TIMING = 1
BP_FLAG_TIME_DOMINANT = 16
BP_FLAG_F32_MFMA = 2
BP_FLAG_BF16_WEIGHTS = 4
BP_FLAG_EXT_CQT_44K = 8
BP_FLAG_F16_CORRECTIONS = 32
BP_FLAG_FP8_CORRECTIONS = 64
BP_FLAG_BLOCKING_WAIT = 128
BP_PCM_F32, BP_PCM_S16, BP_PCM_S24, BP_PCM_S32, BP_PCM_U8, BP_PCM_F64 = range(6)
# what AIFF, CAF and AU files hold (include/basic_pitch_amd_containers.h): big-endian words, signed bytes, G.711
BP_PCM_S16_BE, BP_PCM_S24_BE, BP_PCM_S32_BE, BP_PCM_F32_BE, BP_PCM_F64_BE, BP_PCM_S8, BP_PCM_ULAW, BP_PCM_ALAW = range(6, 14)
# the WAV (format tag, bits per sample) each code stands for; a sample is bits // 8 bytes wide
BP_PCM_WAV = {BP_PCM_U8: (1, 8), BP_PCM_S16: (1, 16), BP_PCM_S24: (1, 24), BP_PCM_S32: (1, 32), BP_PCM_F32: (3, 32),
              BP_PCM_F64: (3, 64), BP_PCM_ULAW: (7, 8), BP_PCM_ALAW: (6, 8)}
# bytes per sample of every code
BP_PCM_WIDTH = {BP_PCM_F32: 4, BP_PCM_S16: 2, BP_PCM_S24: 3, BP_PCM_S32: 4, BP_PCM_U8: 1, BP_PCM_F64: 8, BP_PCM_S16_BE: 2,
                BP_PCM_S24_BE: 3, BP_PCM_S32_BE: 4, BP_PCM_F32_BE: 4, BP_PCM_F64_BE: 8, BP_PCM_S8: 1, BP_PCM_ULAW: 1, BP_PCM_ALAW: 1}
BP_CONTAINER_WAV, BP_CONTAINER_AIFF, BP_CONTAINER_CAF, BP_CONTAINER_AU = 1, 2, 3, 4
BP_ADPCM_IMA_WAV, BP_ADPCM_IMA4 = 1, 2  # include/basic_pitch_amd_adpcm.h: RIFF/WAVE format tag 0x11, CAF `ima4`
BP_N_STAGES = 15
BP_FILES_CLIP_MAX_WINDOWS = 15  # the longest file, in windows, that bp_transcribe_params.clip_batch sends to a batched call
BP_Z_ROW = 448
BP_Z_ROWS = 174
BP_Z_PAD = 56
BP_PYR_STRIDE = 43712

STAGE_NAMES = [
    "pyramid", "filterbank", "contour1", "contour2", "note1", "note2", "onset1", "onset2",
    "zpack", "note", "onset", "contour", "contour_conv1", "contour_conv2", "contour_conv1_edge",
]

_ERR_NAMES = {
    -1: "BP_ERR_INVALID_ARG",
    -2: "BP_ERR_BAD_WEIGHTS",
    -3: "BP_ERR_NO_DEVICE",
    -4: "BP_ERR_HIP",
    -5: "BP_ERR_OUT_OF_MEMORY",
    -6: "BP_ERR_UNSUPPORTED",
    -7: "BP_ERR_BAD_AUDIO",
}


class NativeLibraryError(RuntimeError):
    """The HIP library is missing / unloadable, or a HIP call failed."""


class bp_info(C.Structure):
    _fields_ = [
        ("device_ordinal", C.c_int),
        ("compute_units", C.c_int),
        ("max_windows", C.c_int64),
        ("workspace_bytes", C.c_int64),
        ("arch", C.c_char * 32),
    ]


class bp_stage_buffers(C.Structure):
    _fields_ = [
        ("audio", C.c_void_p),
        ("pyr", C.c_void_p),
        ("lp", C.c_void_p),
        ("mm", C.c_void_p),
        ("c1", C.c_void_p),
        ("contour", C.c_void_p),
        ("n1", C.c_void_p),
        ("note", C.c_void_p),
        ("o1", C.c_void_p),
        ("onset", C.c_void_p),
        ("zp", C.c_void_p),
    ]


class bp_launch_plan_out(C.Structure):
    """What the launchers decide for one chunk (include/basic_pitch_amd.h: bp_launch_plan); every field an int32."""

    _fields_ = [(name, C.c_int32) for name in (
        "pyramid_one_launch", "pyramid_decimate_grid", "pyramid_decimate_grid_cap", "filterbank_fused", "filterbank_grid",
        "conv1_chunks", "conv1_grid", "conv1_prio", "rim_march", "rim_items", "rim_per_side", "rim_items_max", "rim_items_min",
        "rim_ring", "conv2_slots", "conv2_launches", "conv2_windows", "conv2_first_windows", "conv2_first_groups",
        "conv2_first_slabs", "conv2_first_slab_rows", "conv2_first_grid", "conv2_last_windows", "conv2_last_groups",
        "conv2_last_slabs", "conv2_last_slab_rows", "conv2_last_grid", "note_grid", "note_grid_cap", "note_prio", "note_aligned",
        "note_share_spans_pairs", "onset_grid", "onset_grid_cap", "onset_prio", "onset_aligned", "onset_share_spans_pairs",
        "conv2_fused", "fused_cols", "fused_seam_rows", "fused_term_rows", "fused_window_floats", "finish_slabs",
        "finish_slab_rows", "finish_grid")]


class bp_note_params(C.Structure):
    _fields_ = [
        ("onset_threshold", C.c_double),
        ("frame_threshold", C.c_double),
        ("min_freq_hz", C.c_double),
        ("max_freq_hz", C.c_double),
        ("min_note_len", C.c_int32),
        ("infer_onsets", C.c_int32),
        ("melodia_trick", C.c_int32),
        ("include_pitch_bends", C.c_int32),
        ("energy_tol", C.c_int32),
        ("reserved", C.c_int32),
    ]


class bp_flac_stream_layout(C.Structure):
    _fields_ = [
        ("channels", C.c_int32),
        ("sample_rate", C.c_int32),
        ("bits_per_sample", C.c_int32),
        ("min_block", C.c_int32),
        ("max_block", C.c_int32),
        ("n_frames", C.c_int64),
        ("audio_start", C.c_int64),
    ]


class bp_pcm_file_layout(C.Structure):
    _fields_ = [
        ("container", C.c_int32),
        ("format", C.c_int32),
        ("channels", C.c_int32),
        ("sample_rate", C.c_int32),
        ("bits_per_sample", C.c_int32),
        ("reserved", C.c_int32),
        ("n_frames", C.c_int64),
        ("data_start", C.c_int64),
    ]


class bp_adpcm_layout(C.Structure):
    _fields_ = [
        ("container", C.c_int32),
        ("codec", C.c_int32),
        ("channels", C.c_int32),
        ("sample_rate", C.c_int32),
        ("block_bytes", C.c_int32),
        ("block_frames", C.c_int32),
        ("n_frames", C.c_int64),
        ("data_start", C.c_int64),
        ("data_bytes", C.c_int64),
    ]


class bp_adpcm_clip(C.Structure):
    _fields_ = [("file", C.c_void_p), ("nbytes", C.c_size_t)]


class bp_transcribe_params(C.Structure):
    _fields_ = [
        ("notes", bp_note_params),
        ("midi_tempo", C.c_double),
        ("multiple_pitch_bends", C.c_int32),
        ("save_midi", C.c_int32),
        ("save_notes", C.c_int32),
        ("threads", C.c_int32),
        ("host_decode", C.c_int32),
        ("direct_io", C.c_int32),
        ("host_flac", C.c_int32),
        ("clip_batch", C.c_int32),
    ]


class bp_file_report(C.Structure):
    _fields_ = [
        ("status", C.c_int32),
        ("n_note_events", C.c_int32),
        ("n_frames", C.c_int64),
        ("message", C.c_char * 240),
        ("ms_read", C.c_float),
        ("ms_lane_wait", C.c_float),
        ("ms_device", C.c_float),
        ("ms_notes", C.c_float),
        ("ms_write", C.c_float),
    ]


class bp_note_event(C.Structure):
    _fields_ = [
        ("start_s", C.c_double),
        ("end_s", C.c_double),
        ("bend_offset", C.c_int64),
        ("start_frame", C.c_int32),
        ("end_frame", C.c_int32),
        ("pitch_midi", C.c_int32),
        ("n_bends", C.c_int32),
        ("amplitude", C.c_float),
        ("reserved", C.c_int32),
    ]


class bp_sweep_decode(C.Structure):
    """One decode of a sweep (include/basic_pitch_amd_sweep.h): segment `segment` under parameter set `params`."""

    _fields_ = [
        ("segment", C.c_int64),
        ("params", C.c_int32),
        ("reserved", C.c_int32),
    ]


class bp_ref_note(C.Structure):
    """A reference note (include/basic_pitch_amd_score.h): seconds from the start of its segment, a MIDI pitch that may be fractional."""

    _fields_ = [
        ("start_s", C.c_double),
        ("end_s", C.c_double),
        ("pitch_midi", C.c_double),
    ]


class bp_score_params(C.Structure):
    """The tolerances of note-level scoring (include/basic_pitch_amd_score.h); `bp_score_params_default` fills in mir_eval's."""

    _fields_ = [
        ("onset_tolerance_s", C.c_double),
        ("offset_ratio", C.c_double),
        ("offset_min_tolerance_s", C.c_double),
        ("pitch_tolerance_cents", C.c_double),
        ("strict", C.c_int32),
        ("reserved", C.c_int32),
    ]


class bp_note_score(C.Structure):
    """The counts of one scored decode (include/basic_pitch_amd_score.h)."""

    _fields_ = [
        ("n_ref", C.c_int32),
        ("n_est", C.c_int32),
        ("matched_onset", C.c_int32),
        ("matched_offset", C.c_int32),
    ]


class bp_frame_score(C.Structure):
    """The frame-level counts of one scored decode (include/basic_pitch_amd_frame_score.h)."""

    _fields_ = [
        ("n_frames", C.c_int64),
        ("ref_frames", C.c_int64),
        ("est_frames", C.c_int64),
        ("true_pos", C.c_int64),
        ("e_sub", C.c_int64),
    ]


class bp_mp_params(C.Structure):
    """One parameter set of multi-pitch picking (include/basic_pitch_amd_multipitch.h); `bp_mp_params_default` fills it in."""

    _fields_ = [
        ("threshold", C.c_float),
        ("min_bin", C.c_int32),
        ("max_bin", C.c_int32),
        ("reserved", C.c_int32),
    ]


class bp_f0_point(C.Structure):
    """One f0 peak of a contour row (include/basic_pitch_amd_multipitch.h)."""

    _fields_ = [
        ("frame", C.c_int32),
        ("salience", C.c_float),
        ("pitch_midi", C.c_double),
    ]


class bp_melody_params(C.Structure):
    """One parameter set of the melody decode (include/basic_pitch_amd_melody.h); `bp_melody_params_default` fills it in."""

    _fields_ = [
        ("threshold", C.c_float),
        ("jump_penalty", C.c_float),
        ("voicing_penalty", C.c_float),
        ("max_jump", C.c_int32),
        ("min_bin", C.c_int32),
        ("max_bin", C.c_int32),
        ("reserved", C.c_int32 * 2),
    ]


class bp_melody_point(C.Structure):
    """The melody record of one contour row (include/basic_pitch_amd_melody.h); bin -1: unvoiced."""

    _fields_ = [
        ("bin", C.c_int32),
        ("salience", C.c_float),
        ("pitch_midi", C.c_double),
    ]


class bp_melody_score(C.Structure):
    """The counts the melody measures are formed from (include/basic_pitch_amd_melody.h)."""

    _fields_ = [
        ("n_frames", C.c_int64),
        ("ref_voiced", C.c_int64),
        ("est_voiced", C.c_int64),
        ("both_voiced", C.c_int64),
        ("pitch_ok", C.c_int64),
        ("chroma_ok", C.c_int64),
    ]


class bp_align_state(C.Structure):
    """One state of a score (include/basic_pitch_amd_align.h): bit p of `active` is pitch 21 + p, `begins` a subset of it."""

    _fields_ = [
        ("active", C.c_uint64 * 2),
        ("begins", C.c_uint64 * 2),
        ("earliest", C.c_int32),
        ("latest", C.c_int32),
    ]


class bp_align_params(C.Structure):
    """The parameters of forced alignment (include/basic_pitch_amd_align.h); `bp_align_params_default` fills them in."""

    _fields_ = [
        ("threshold_q", C.c_int32),
        ("onset_weight", C.c_int32),
        ("reserved", C.c_int32 * 2),
    ]


class bp_beat_params(C.Structure):
    """The parameters of tempo and beats (include/basic_pitch_amd_beat.h), the prior table among them;
    `bp_beat_params_default` fills them in."""

    _fields_ = [
        ("threshold_q", C.c_int32),
        ("min_pitch", C.c_int32),
        ("max_pitch", C.c_int32),
        ("lag_min", C.c_int32),
        ("lag_max", C.c_int32),
        ("tightness", C.c_int32),
        ("reserved", C.c_int32 * 2),
        ("prior", C.c_int32 * 257),
        ("reserved_tail", C.c_int32),
    ]


class bp_beat_summary(C.Structure):
    """Tempo and beats of one segment (include/basic_pitch_amd_beat.h): status 1 a NaN, 2 no pulse."""

    _fields_ = [
        ("status", C.c_int32),
        ("period", C.c_int32),
        ("n_beats", C.c_int64),
        ("score", C.c_int64),
        ("period_refined", C.c_double),
    ]


class bp_chord_params(C.Structure):
    """The parameters of chords and key (include/basic_pitch_amd_chord.h), the state table and the key profiles among them;
    `bp_chord_params_default` fills them in."""

    _fields_ = [
        ("threshold_q", C.c_int32),
        ("min_pitch", C.c_int32),
        ("max_pitch", C.c_int32),
        ("n_states", C.c_int32),
        ("switch_penalty", C.c_int32),
        ("reserved", C.c_int32 * 3),
        ("bias", C.c_int32 * 64),
        ("weights", (C.c_int32 * 12) * 64),
        ("key_profile", (C.c_int32 * 12) * 2),
    ]


class bp_chord_summary(C.Structure):
    """Chords and key of one segment (include/basic_pitch_amd_chord.h): status 1 a NaN, 2 nothing sounds."""

    _fields_ = [
        ("status", C.c_int32),
        ("key", C.c_int32),
        ("n_units", C.c_int32),
        ("n_changes", C.c_int32),
        ("score", C.c_int64),
        ("key_score", C.c_int64),
    ]


class bp_sync_params(C.Structure):
    """The parameters of the synchronisation of two segments (include/basic_pitch_amd_sync.h); `bp_sync_params_default` fills
    them in."""

    _fields_ = [
        ("threshold_q", C.c_int32),
        ("min_pitch", C.c_int32),
        ("max_pitch", C.c_int32),
        ("hop", C.c_int32),
        ("band", C.c_int32),
        ("reserved", C.c_int32 * 3),
    ]


class bp_sync_pair(C.Structure):
    """One pair of segment indices of a synchronisation job (include/basic_pitch_amd_sync.h)."""

    _fields_ = [
        ("a", C.c_int32),
        ("b", C.c_int32),
    ]


class bp_sync_summary(C.Structure):
    """The synchronisation of one pair (include/basic_pitch_amd_sync.h): status 1 a NaN, 2 a segment without rows."""

    _fields_ = [
        ("status", C.c_int32),
        ("units_a", C.c_int32),
        ("units_b", C.c_int32),
        ("n_path", C.c_int32),
        ("path_first", C.c_int64),
        ("total", C.c_int64),
    ]


class bp_stream_update(C.Structure):
    """One stream of `bp_streams_candidates` (include/basic_pitch_amd_update.h): `stream` and `held_rows` in, the rest out."""

    _fields_ = [
        ("stream", C.c_void_p),
        ("held_rows", C.c_int64),
        ("first_row", C.c_int64),
        ("n_rows", C.c_int64),
        ("new_row", C.c_int64),
        ("note_offset", C.c_int64),
        ("bits_offset", C.c_int64),
        ("status", C.c_int),
    ]


class bp_stream_events(C.Structure):
    """One stream of `bp_streams_events` (include/basic_pitch_amd_stream_events.h): `stream` in, the rest out."""

    _fields_ = [
        ("stream", C.c_void_p),
        ("first_row", C.c_int64),
        ("n_rows", C.c_int64),
        ("status", C.c_int),
    ]


# every symbol include/basic_pitch_amd.h declares (tests check they are all exported)
EXPORTED_SYMBOLS = [
    "bp_create",
    "bp_destroy",
    "bp_last_error",
    "bp_infer",
    "bp_infer_async",
    "bp_infer_track",
    "bp_infer_tracks",
    "bp_resampled_length",
    "bp_resample",
    "bp_infer_pcm",
    "bp_infer_pcm_raw",
    "bp_host_alloc",
    "bp_host_free",
    "bp_files_release_buffers",
    "bp_files_direct_reads",
    "bp_files_read_probe",
    "bp_files_batched",
    "bp_files_batch_probe",
    "bp_track_n_windows",
    "bp_handle_track_n_windows",
    "bp_handle_track_n_frames",
    "bp_handle_window_samples",
    "bp_handle_sample_rate",
    "bp_handle_resampled_length",
    "bp_track_n_frames",
    "bp_set_stream",
    "bp_synchronize",
    "bp_get_info",
    "bp_get_stage_ms",
    "bp_run_stage",
    "bp_launch_plan",
    "bp_pyramid_layout",
    "bp_version",
    "bp_device_count",
    "bp_note_params_default",
    "bp_notes_decode",
    "bp_note_candidates",
    "bp_infer_pcm_raw_candidates",
    "bp_track_maps",
    "bp_notes_decode_candidates",
    "bp_notes_last_error",
    "bp_flac_info",
    "bp_flac_decode",
    "bp_flac_layout",
    "bp_flac_decode_device",
    "bp_infer_flac",
    "bp_infer_flac_candidates",
    "bp_audio_last_error",
    "bp_transcribe_params_default",
    "bp_transcribe_files",
    "bp_notes_to_midi",
    "bp_notes_to_csv",
    "bp_wav_info",
    "bp_wav_decode",
    "bp_files_last_error",
    "bp_stream_open",
    "bp_stream_push",
    "bp_stream_finish",
    "bp_streams_push",
    "bp_stream_close",
    "bp_stream_rows_bound",
    "bp_stream_state_bytes",
    "bp_stream_rows_after",
]
# every symbol include/basic_pitch_amd_live.h declares
LIVE_SYMBOLS = [
    "bp_stream_peek",
    "bp_streams_peek",
    "bp_stream_keep",
    "bp_stream_candidates",
]
# every symbol include/basic_pitch_amd_rolling.h declares
ROLLING_SYMBOLS = [
    "bp_stream_keep_rolling",
    "bp_stream_horizon_first_row",
    "bp_stream_candidates_rolling",
    "bp_stream_rolling_maps",
    "bp_notes_decode_candidates_at",
]
# every symbol include/basic_pitch_amd_update.h declares (bound in basic_pitch_amd/streaming.py)
UPDATE_SYMBOLS = [
    "bp_streams_update_layout",
    "bp_streams_candidates",
]
# every symbol include/basic_pitch_amd_stream_events.h declares (bound in basic_pitch_amd/streaming.py)
STREAM_EVENTS_SYMBOLS = [
    "bp_streams_events_layout",
    "bp_streams_events",
]
# every symbol include/basic_pitch_amd_clips.h declares (bound in basic_pitch_amd/clips.py)
CLIPS_SYMBOLS = [
    "bp_clips_row_offsets",
    "bp_infer_clips_candidates",
]
# every symbol include/basic_pitch_amd_events.h declares (bound in basic_pitch_amd/events.py)
EVENTS_SYMBOLS = [
    "bp_events_capacity",
    "bp_infer_clips_events",
    "bp_note_events_from_maps",
]
# every symbol include/basic_pitch_amd_sweep.h declares (bound in basic_pitch_amd/sweep.py)
SWEEP_SYMBOLS = [
    "bp_note_events_sweep",
    "bp_infer_clips_events_sweep",
]
# every symbol include/basic_pitch_amd_score.h declares (bound in basic_pitch_amd/score.py)
SCORE_SYMBOLS = [
    "bp_score_params_default",
    "bp_score_note_events",
    "bp_note_events_sweep_score",
    "bp_infer_clips_events_sweep_score",
]
# every symbol include/basic_pitch_amd_frame_score.h declares (bound in basic_pitch_amd/frame_score.py)
FRAME_SCORE_SYMBOLS = [
    "bp_score_note_frames",
    "bp_note_events_sweep_frame_score",
    "bp_infer_clips_events_sweep_frame_score",
]
# every symbol include/basic_pitch_amd_multipitch.h declares (bound in basic_pitch_amd/multipitch.py)
MULTIPITCH_SYMBOLS = [
    "bp_mp_params_default",
    "bp_multipitch_rows",
    "bp_score_f0_frames",
    "bp_multipitch_from_maps",
    "bp_infer_clips_multipitch",
    "bp_multipitch_sweep_frame_score",
    "bp_infer_clips_multipitch_sweep_frame_score",
]
# every symbol include/basic_pitch_amd_melody.h declares (bound in basic_pitch_amd/melody.py)
MELODY_SYMBOLS = [
    "bp_melody_params_default",
    "bp_melody_rows",
    "bp_score_melody_frames",
    "bp_melody_from_maps",
    "bp_infer_clips_melody",
    "bp_melody_sweep_score",
    "bp_infer_clips_melody_sweep_score",
]
# every symbol include/basic_pitch_amd_align.h declares (bound in basic_pitch_amd/align.py)
ALIGN_SYMBOLS = [
    "bp_align_params_default",
    "bp_align_rows",
    "bp_align_from_maps",
    "bp_infer_clips_align",
]
# every symbol include/basic_pitch_amd_beat.h declares (bound in basic_pitch_amd/beat.py)
BEAT_SYMBOLS = [
    "bp_beat_params_default",
    "bp_beat_prior",
    "bp_beats_capacity",
    "bp_beat_rows",
    "bp_beats_from_maps",
    "bp_infer_clips_beats",
]
# every symbol include/basic_pitch_amd_chord.h declares (bound in basic_pitch_amd/chord.py)
CHORD_SYMBOLS = [
    "bp_chord_params_default",
    "bp_chord_templates",
    "bp_chord_key_profiles",
    "bp_chord_rows",
    "bp_chords_from_maps",
    "bp_infer_clips_chords",
]
# every symbol include/basic_pitch_amd_sync.h declares (bound in basic_pitch_amd/sync.py)
SYNC_SYMBOLS = [
    "bp_sync_params_default",
    "bp_sync_rows",
    "bp_sync_from_maps",
    "bp_infer_clips_sync",
]
# every symbol include/basic_pitch_amd_flac_clips.h declares (bound in basic_pitch_amd/flac_clips.py)
FLAC_CLIPS_SYMBOLS = [
    "bp_flac_clips_row_offsets",
    "bp_flac_clips_decode_device",
    "bp_infer_flac_clips_candidates",
    "bp_infer_flac_clips_events",
]
# every symbol include/basic_pitch_amd_containers.h declares (bound below; basic_pitch_amd/audio.py pcm_raw is their numpy twin)
CONTAINERS_SYMBOLS = [
    "bp_pcm_file_layout_of",
    "bp_pcm_file_decode",
]
# every symbol include/basic_pitch_amd_adpcm.h declares (bound below)
ADPCM_SYMBOLS = [
    "bp_adpcm_layout_of",
    "bp_adpcm_decode",
    "bp_adpcm_decode_device",
    "bp_infer_adpcm",
    "bp_infer_adpcm_candidates",
    "bp_infer_adpcm_clips_events",
]
# status values of a clip in those calls, beside 0, 1 and 2 of the PCM clips calls
BP_CLIP_FLAC_HOST = 3    # left to the host decoder, known before anything is queued: no rows
BP_CLIP_FLAC_FAILED = 4  # the device decoder could not follow the stream

_lib: Optional[C.CDLL] = None


def load_library(path: Optional[str] = None) -> C.CDLL:
    """dlopen the in-tree library and declare argtypes.  Raises NativeLibraryError if absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("BASIC_PITCH_AMD_LIB") or _build.LIB_PATH
    if not os.path.exists(p):
        raise NativeLibraryError(
            f"{p} not found. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc, gfx950). basic_pitch_amd has no CPU fallback."
        )
    # ONE HIP runtime per process.  PyTorch's libraries ask for "libamdhip64.so" (and find the copy bundled in torch/lib),
    # this library for "libamdhip64.so.7" (the system's /opt/rocm copy); both files carry the SONAME libamdhip64.so.7.  When
    # torch loads first, this library's request matches the SONAME of the copy already in the process.  The other way
    # round torch's request matched nothing and a SECOND runtime was loaded — whichever initialised second then saw no
    # device (measured: build() followed by smoke() in one process).  Loading the runtime by torch's name first puts that
    # name on the link map, so a later `import torch` reuses it.
    try:
        C.CDLL("libamdhip64.so", mode=C.RTLD_GLOBAL)
    except OSError:
        pass
    try:
        lib = C.CDLL(p)
    except OSError as e:  # missing libamdhip64 etc.
        raise NativeLibraryError(f"cannot load {p}: {e}") from e
    vp, i64, fp = C.c_void_p, C.c_int64, C.c_void_p
    lib.bp_create.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_uint, i64, C.POINTER(vp)]
    lib.bp_create.restype = C.c_int
    lib.bp_destroy.argtypes = [vp]
    lib.bp_destroy.restype = None
    lib.bp_last_error.argtypes = [vp]
    lib.bp_last_error.restype = C.c_char_p
    lib.bp_infer.argtypes = [vp, fp, i64, fp, fp, fp, C.c_int]
    lib.bp_infer.restype = C.c_int
    lib.bp_infer_async.argtypes = [vp, fp, i64, fp, fp, fp]
    lib.bp_infer_async.restype = C.c_int
    lib.bp_infer_track.argtypes = [vp, fp, i64, fp, fp, fp, C.c_int]
    lib.bp_infer_track.restype = C.c_int
    lib.bp_infer_tracks.argtypes = [vp, i64, vp, vp, vp, vp, vp, C.c_int]
    lib.bp_infer_tracks.restype = C.c_int
    lib.bp_resampled_length.argtypes = [i64, C.c_int]
    lib.bp_resampled_length.restype = i64
    lib.bp_resample.argtypes = [vp, fp, i64, C.c_int, C.c_int, fp, C.c_int]
    lib.bp_resample.restype = C.c_int
    lib.bp_infer_pcm.argtypes = [vp, fp, i64, C.c_int, C.c_int, fp, fp, fp, C.c_int]
    lib.bp_infer_pcm.restype = C.c_int
    lib.bp_infer_pcm_raw.argtypes = [vp, vp, C.c_int, i64, C.c_int, C.c_int, fp, fp, fp, C.c_int]
    lib.bp_infer_pcm_raw.restype = C.c_int
    lib.bp_flac_layout.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(bp_flac_stream_layout)]
    lib.bp_flac_layout.restype = C.c_int
    lib.bp_flac_decode_device.argtypes = [vp, C.c_char_p, C.c_size_t, vp, i64, C.POINTER(i64)]
    lib.bp_flac_decode_device.restype = C.c_int
    lib.bp_infer_flac.argtypes = [vp, C.c_char_p, C.c_size_t, fp, fp, fp, C.c_int]
    lib.bp_infer_flac.restype = C.c_int
    lib.bp_host_alloc.argtypes = [C.c_size_t]
    lib.bp_host_alloc.restype = C.c_void_p
    lib.bp_host_free.argtypes = [C.c_void_p]
    lib.bp_host_free.restype = None
    lib.bp_files_release_buffers.argtypes = []
    lib.bp_files_release_buffers.restype = None
    lib.bp_files_direct_reads.argtypes = []
    lib.bp_files_direct_reads.restype = C.c_int64
    lib.bp_files_read_probe.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
    lib.bp_files_read_probe.restype = C.c_int64
    lib.bp_files_batched.argtypes = []
    lib.bp_files_batched.restype = C.c_int64
    lib.bp_files_batch_probe.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(C.c_char_p), i64, C.POINTER(bp_transcribe_params),
                                         C.POINTER(C.c_int32)]
    lib.bp_files_batch_probe.restype = C.c_int
    lib.bp_handle_track_n_windows.argtypes = [vp, i64]
    lib.bp_handle_track_n_windows.restype = i64
    lib.bp_handle_track_n_frames.argtypes = [vp, i64]
    lib.bp_handle_track_n_frames.restype = i64
    lib.bp_handle_window_samples.argtypes = [vp]
    lib.bp_handle_window_samples.restype = i64
    lib.bp_handle_sample_rate.argtypes = [vp]
    lib.bp_handle_sample_rate.restype = C.c_int
    lib.bp_handle_resampled_length.argtypes = [vp, i64, C.c_int]
    lib.bp_handle_resampled_length.restype = i64
    lib.bp_track_n_windows.argtypes = [i64]
    lib.bp_track_n_windows.restype = i64
    lib.bp_track_n_frames.argtypes = [i64]
    lib.bp_track_n_frames.restype = i64
    lib.bp_set_stream.argtypes = [vp, vp]
    lib.bp_set_stream.restype = C.c_int
    lib.bp_synchronize.argtypes = [vp]
    lib.bp_synchronize.restype = C.c_int
    lib.bp_get_info.argtypes = [vp, C.POINTER(bp_info)]
    lib.bp_get_info.restype = C.c_int
    lib.bp_get_stage_ms.argtypes = [vp, C.POINTER(C.c_float), C.c_int]
    lib.bp_get_stage_ms.restype = C.c_int
    lib.bp_run_stage.argtypes = [vp, C.c_int, C.POINTER(bp_stage_buffers), i64]
    lib.bp_run_stage.restype = C.c_int
    lib.bp_launch_plan.argtypes = [i64, C.c_int, C.c_uint, C.POINTER(bp_launch_plan_out)]
    lib.bp_launch_plan.restype = C.c_int
    lib.bp_pyramid_layout.argtypes = [C.c_int, C.POINTER(i64), C.POINTER(i64)]
    lib.bp_pyramid_layout.restype = C.c_int
    lib.bp_device_count.argtypes = []
    lib.bp_device_count.restype = C.c_int
    lib.bp_version.argtypes = []
    lib.bp_version.restype = C.c_char_p
    lib.bp_note_params_default.argtypes = [C.POINTER(bp_note_params)]
    lib.bp_note_params_default.restype = None
    lib.bp_notes_decode.argtypes = [
        vp, vp, vp, i64, C.POINTER(bp_note_params), vp, i64, vp, i64, C.POINTER(i64), C.POINTER(i64)
    ]
    lib.bp_notes_decode.restype = C.c_int
    lib.bp_note_candidates.argtypes = [vp, vp, vp, vp, i64, C.POINTER(bp_note_params), C.c_int, vp, vp, vp, C.POINTER(C.c_int)]
    lib.bp_note_candidates.restype = C.c_int
    lib.bp_infer_pcm_raw_candidates.argtypes = [
        vp, vp, C.c_int, i64, C.c_int, C.c_int, C.POINTER(bp_note_params), vp, vp, vp, C.POINTER(C.c_int)
    ]
    lib.bp_infer_pcm_raw_candidates.restype = C.c_int
    lib.bp_track_maps.argtypes = [vp, i64, vp, vp, vp, C.c_int]
    lib.bp_track_maps.restype = C.c_int
    lib.bp_notes_decode_candidates.argtypes = [
        vp, vp, vp, i64, C.POINTER(bp_note_params), vp, i64, vp, i64, C.POINTER(i64), C.POINTER(i64)
    ]
    lib.bp_notes_decode_candidates.restype = C.c_int
    lib.bp_notes_decode_candidates_at.argtypes = [
        vp, vp, vp, i64, i64, vp, vp, i64, vp, i64, C.POINTER(i64), C.POINTER(i64)
    ]
    lib.bp_notes_decode_candidates_at.restype = C.c_int
    lib.bp_notes_last_error.argtypes = []
    lib.bp_notes_last_error.restype = C.c_char_p
    pi = C.POINTER(C.c_int)
    lib.bp_flac_info.argtypes = [C.c_char_p, C.c_size_t, pi, pi, pi, C.POINTER(i64)]
    lib.bp_flac_info.restype = C.c_int
    lib.bp_flac_decode.argtypes = [C.c_char_p, C.c_size_t, fp, i64, C.POINTER(i64)]
    lib.bp_flac_decode.restype = C.c_int
    lib.bp_audio_last_error.argtypes = []
    lib.bp_audio_last_error.restype = C.c_char_p
    lib.bp_transcribe_params_default.argtypes = [C.POINTER(bp_transcribe_params)]
    lib.bp_transcribe_params_default.restype = None
    lib.bp_transcribe_files.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(C.c_char_p), i64, C.c_char_p,
                                        C.POINTER(bp_transcribe_params), C.POINTER(bp_file_report)]
    lib.bp_transcribe_files.restype = C.c_int
    lib.bp_notes_to_midi.argtypes = [C.c_void_p, i64, C.c_void_p, C.c_int, C.c_double, C.c_void_p, i64]
    lib.bp_notes_to_midi.restype = i64
    lib.bp_notes_to_csv.argtypes = [C.c_void_p, i64, C.c_void_p, C.c_void_p, i64]
    lib.bp_notes_to_csv.restype = i64
    lib.bp_wav_info.argtypes = [C.c_char_p, C.c_size_t, pi, pi, pi, C.POINTER(i64)]
    lib.bp_wav_info.restype = C.c_int
    lib.bp_wav_decode.argtypes = [C.c_char_p, C.c_size_t, fp, i64, C.POINTER(i64)]
    lib.bp_wav_decode.restype = C.c_int
    lib.bp_pcm_file_layout_of.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(bp_pcm_file_layout)]
    lib.bp_pcm_file_layout_of.restype = C.c_int
    lib.bp_pcm_file_decode.argtypes = [C.c_char_p, C.c_size_t, fp, i64, C.POINTER(i64)]
    lib.bp_pcm_file_decode.restype = C.c_int
    lib.bp_adpcm_layout_of.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(bp_adpcm_layout)]
    lib.bp_adpcm_layout_of.restype = C.c_int
    lib.bp_adpcm_decode.argtypes = [C.c_char_p, C.c_size_t, vp, i64, C.POINTER(i64)]
    lib.bp_adpcm_decode.restype = C.c_int
    lib.bp_adpcm_decode_device.argtypes = [vp, C.c_char_p, C.c_size_t, vp, i64, C.POINTER(i64)]
    lib.bp_adpcm_decode_device.restype = C.c_int
    lib.bp_infer_adpcm.argtypes = [vp, C.c_char_p, C.c_size_t, fp, fp, fp, C.c_int]
    lib.bp_infer_adpcm.restype = C.c_int
    lib.bp_infer_adpcm_candidates.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(bp_note_params), vp, vp, vp, C.POINTER(C.c_int)]
    lib.bp_infer_adpcm_candidates.restype = C.c_int
    lib.bp_infer_adpcm_clips_events.argtypes = [vp, i64, C.POINTER(bp_adpcm_clip), vp, vp, i64, vp, i64, vp, vp]
    lib.bp_infer_adpcm_clips_events.restype = C.c_int
    lib.bp_files_last_error.argtypes = []
    lib.bp_files_last_error.restype = C.c_char_p
    if path is None:
        _lib = lib
    return lib


def bind(lib: C.CDLL, prototypes: dict) -> C.CDLL:
    """Declare `prototypes` (name -> (restype, argtypes), as a header declares them) on a loaded library."""
    for name, (restype, argtypes) in prototypes.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def check(lib: C.CDLL, handle, rc: int, what: str) -> None:
    """Map a negative bp_status to the exception the reference's callers would see."""
    if rc == BP_OK:
        return
    msg = lib.bp_last_error(handle)
    text = f"{what}: {_ERR_NAMES.get(rc, rc)}: {msg.decode(errors='replace') if msg else ''}"
    if rc in (-1, -2, -6, -7):  # -7: undecodable audio (what audio.read_audio raises ValueError for)
        raise ValueError(text)  # reference: ValueError for bad model / bad shapes (inference.py:148-154)
    raise NativeLibraryError(text)
