"""ctypes binding of include/toucan_tts.h (libtoucan_hip.so).

The library is mandatory: there is no CPU or PyTorch fallback anywhere in the product path.
``lib()`` raises if the shared object is missing or does not export the full ABI.
"""
import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TOUCAN_HIP_LIB") or os.path.join(_PKG, "libtoucan_hip.so")  # the override selects another build of the library, e.g. the parent commit's

MODE_LINEAR, MODE_GLU, MODE_GATED, MODE_COUPLING = 0, 1, 2, 3
ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2
PRE_NONE, PRE_LRELU, PRE_SNAKE = 0, 1, 2
COMPUTE_F32, COMPUTE_BF16, COMPUTE_F16 = 0, 1, 2
COMPUTE_F32X3 = 3  # fp32 tensors, every product as three fp16 MFMAs on split operands (include/toucan_tts.h TTS_COMPUTE_F32X3)

_p = C.c_void_p
_i = C.c_int32
_f = C.c_float


class TtsTile(C.Structure):
    _fields_ = [("row0", _i), ("seq_begin", _i), ("seq_end", _i), ("seq_id", _i)]


class TtsConvDesc(C.Structure):
    _fields_ = [
        ("x", _p), ("ldx", _i), ("cin", _i),
        ("w", _p), ("cin_pad", _i), ("wn", _i), ("half_pad", _i),
        ("bias", _p),
        ("y", _p), ("ldy", _i), ("cout", _i),
        ("taps", _i), ("dil", _i), ("pad_left", _i),
        ("pre_act", _i), ("pre_slope", _f),
        ("snake_alpha", _p), ("snake_beta", _p), ("snake_filt", _p),
        ("mode", _i), ("act", _i), ("alpha", _f),
        ("seqvec", _p), ("ld_seqvec", _i),
        ("preadd", _p), ("ld_preadd", _i),
        ("res", _p), ("ld_res", _i), ("res_scale", _f),
        ("aux", _p), ("ld_aux", _i),
        ("accumulate", _i),
        ("compute", _i),
        ("io_flags", _i),
        ("tiles", _p), ("n_tiles", _i), ("tile_rows", _i),
    ]


class TtsResblockDesc(C.Structure):
    _fields_ = [
        ("x", _p), ("ldx", _i),
        ("y", _p), ("ldy", _i),
        ("c", _i), ("taps", _i), ("dil", _i),
        ("w1", _p), ("b1", _p),
        ("w2", _p), ("b2", _p),
        ("act", _i), ("slope", _f),
        ("alpha1", _p), ("beta1", _p), ("alpha2", _p), ("beta2", _p), ("filt", _p),
        ("alpha", _f), ("res_scale", _f), ("accumulate", _i),
        ("io_bf16", _i),
        ("tiles", _p), ("n_tiles", _i), ("tile_rows", _i),
        ("compute", _i),
        ("fir_tab", _p),
    ]


class TtsWavenetDesc(C.Structure):
    _fields_ = [
        ("hs_in", _p), ("ld_in", _i),
        ("hs_out", _p), ("ld_out", _i),
        ("cond", _p), ("ld_cond", _i),
        ("w1", _p), ("b1", _p),
        ("w2", _p), ("b2", _p),
        ("cout2", _i),
        ("compute", _i),
        ("tiles", _p), ("n_tiles", _i), ("tile_rows", _i),
    ]


class TtsFfnDesc(C.Structure):
    _fields_ = [
        ("x", _p), ("ldx", _i),
        ("y", _p), ("ldy", _i),
        ("rows", _i), ("channels", _i),
        ("ln_g", _p), ("ln_b", _p),
        ("w", _p), ("b2", _p),
        ("post_g", _p), ("post_b", _p),
        ("hidden", _i), ("compute", _i),
        ("alpha", _f), ("eps", _f),
    ]


class TtsConfig(C.Structure):
    _fields_ = [("multilingual", _i), ("multispeaker", _i), ("vocoder", _i), ("precision", _i), ("small_tile_blocks", _i), ("post_bias", _f)]


IO_X_BF16, IO_Y_BF16, IO_RES_BF16, IO_F16 = 1, 2, 4, 8
IO_SPLIT_K = 16  # tts_conv1d, fp32: the caller accepts the split-K form on small grids (the frame stages of the fp32 acoustic model do)
IO_SPLIT_K_ALWAYS = 32  # ... at every grid size (its phoneme stages: one arithmetic upstream of the rounded durations whatever the batch)
IO_POLYPHASE = 64  # tts_conv1d, wide tile (tile_rows 256): a 3-tap polyphase up-sampler whose structural zeros the kernel leaves out
ATT_KEY_SPLIT, ATT_KEY_SPLIT_ALWAYS = 1, 2  # tts_relpos_attention flags (include/toucan_tts.h)

# symbol -> (restype, argtypes); mirrors include/toucan_tts.h one to one
PROTOTYPES = {
    "tts_last_error": (C.c_char_p, []),
    "tts_abi_version": (C.c_int, []),
    "tts_diag_queue_nonzero": (C.c_int, []),
    "tts_diag_queue_slots_used": (C.c_int, []),
    "tts_conv1d_tile_rows": (C.c_int, [_i, _i]),
    "tts_conv1d_n_tile": (C.c_int, [_i, _i]),
    "tts_conv1d_small_tile_rows": (C.c_int, [_i, _i, _i]),
    "tts_conv1d": (C.c_int, [C.POINTER(TtsConvDesc), _p]),
    "tts_resblock_step": (C.c_int, [C.POINTER(TtsResblockDesc), _p]),
    "tts_resblock_tile_rows": (C.c_int, [_i]),
    "tts_snake_fir_table": (C.c_int, [_p, _p]),
    "tts_wavenet_layer": (C.c_int, [C.POINTER(TtsWavenetDesc), _p]),
    "tts_ffn_fused": (C.c_int, [C.POINTER(TtsFfnDesc), _p]),
    "tts_layernorm": (C.c_int, [_p, _i, _p, _i, _p, _p, _i, _i, _f, _p]),
    "tts_cond_layernorm": (C.c_int, [_p, _i, _p, _i, _p, _p, _i, _p, _i, _i, _p]),
    "tts_cln_mlp_weight_floats": (C.c_int64, [_i, _i]),
    "tts_cln_mlp": (C.c_int, [_p, _i, _i, _i, _p, _i, _p, _p]),
    "tts_l2_normalize": (C.c_int, [_p, _p, _i, _i, _p]),
    "tts_groupnorm": (C.c_int, [_p, _i, _p, _i, _p, _p, _i, _i, _f, _i, _p, _i, _p, _p, _i, _i, _p, _p]),
    "tts_groupnorm_workspace_floats": (C.c_int64, [_i, _i, _i]),
    "tts_relpos_attention": (C.c_int, [_p, _i, _p, _i, _p, _p, _p, _i, _i, _i, _p, _i, _i, _i, _p]),
    "tts_relpos_attention_f16": (C.c_int, [_p, _i, _p, _i, _p, _p, _p, _i, _i, _i, _p, _i, _i, _p]),
    "tts_dwconv_swish": (C.c_int, [_p, _i, _p, _i, _p, _p, _i, _i, _p, _i, _i, _p]),
    "tts_duration_from_log": (C.c_int, [_p, _p, _i, _p]),
    "tts_prosody_control": (C.c_int, [_p, _i, _p, _p, _p, _p, _p, _i, _f, _f, _f, _f, _p]),
    "tts_length_regulate": (C.c_int, [_p, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _i, _p, _i, _f, _p]),
    "tts_glow_invconv_actnorm": (C.c_int, [_p, _i, _i, _i, _p, _p, _p, _p]),
    "tts_snake_aa": (C.c_int, [_p, _i, _p, _i, _p, _p, _p, _i, _p, _i, _i, _i, _p]),
    "tts_conv_post": (C.c_int, [_p, _i, _i, _p, _f, _i, _f, _p, _p, _i, _i, _i, _p]),
    "tts_conv_post_snake_tile_rows": (C.c_int, []),
    "tts_conv_post_snake": (C.c_int, [_p, _i, _i, _p, _f, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "tts_gather_rows": (C.c_int, [_p, _i, _p, _p, _i, _i, _i, _p]),
    # per-speaker path (csrc/style.hip)
    "tts_gru_layer": (C.c_int, [_p, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _i, _p]),
    "tts_style_tokens": (C.c_int, [_p, _p, _p, _i, _i, _i, _i, _p, _p]),
    "tts_complex_magnitude": (C.c_int, [_p, _i, _p, _i, _i, _i, _p]),
    "tts_log10_floor": (C.c_int, [_p, _i, _p, _i, _i, _i, _f, _p]),
    # stage API (csrc/pipeline.hip)
    "tts_create": (C.c_int, [C.POINTER(TtsConfig), C.POINTER(_p)]),
    "tts_destroy": (C.c_int, [_p]),
    "tts_load_weights": (C.c_int, [_p, C.c_char_p, _p, C.POINTER(C.c_int64), _i, _i]),
    "tts_workspace_bytes": (C.c_int64, [_p, _i, _i, _i]),
    "tts_workspace_claimed": (C.c_int64, [_p]),
    "tts_table_stats": (C.c_int, [_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tts_encoder": (C.c_int, [_p, _p, _p, _p, _p, _i, _p]),
    "tts_variance_predictors": (C.c_int, [_p, _p, _p, _p, _p]),
    "tts_control_and_regulate": (C.c_int, [_p, _f, _f, _f, _f, _p, _p]),
    "tts_decoder": (C.c_int, [_p, _p]),
    "tts_postnet": (C.c_int, [_p, _p]),
    "tts_postflow": (C.c_int, [_p, _p, _p]),
    "tts_mel": (C.c_int, [_p, C.POINTER(_p), C.POINTER(_i), _p, _p]),
    "tts_prosody": (C.c_int, [_p, C.POINTER(_p), C.POINTER(_p), C.POINTER(_p)]),
    "tts_copy_mel": (C.c_int, [_p, _p, _i, _p]),
    "tts_copy_prosody": (C.c_int, [_p, _p, _p, _p, _p]),
    "tts_profile": (C.c_int, [_p, _i, C.c_char_p]),
    "tts_profile_count": (_i, [_p]),
    "tts_profile_read": (C.c_int, [_p, _i, C.c_char_p, _i, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "tts_vocoder_bigvgan": (C.c_int, [_p, _p, _i, _p, _p, _i, _p, _p]),
    "tts_vocoder_hifigan": (C.c_int, [_p, _p, _i, _p, _p, _i, _p, _p]),
    "tts_synthesize_batch": (C.c_int, [_p, _p, _p, _p, _p, _i, _p, _p, _p, _f, _f, _f, _f, _p, _p, _p, _p, C.c_int64, C.POINTER(C.c_int64), _p]),
}

# symbol -> (restype, argtypes); mirrors include/toucan_align.h (the prosody cloner's kernels, csrc/align.hip) one to one
ALIGN_PROTOTYPES = {
    "tts_relu_affine": (C.c_int, [_p, _i, _p, _i, _i, _i, _p, _p, _p]),
    "tts_lstm_recurrence": (C.c_int, [_p, _i, _p, _p, _p, _p, _p, _p, _i, _p, _p, _i, _i, _i, _p]),
    "tts_mas_durations": (C.c_int, [_p, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p, _p]),
    "tts_frame_energy": (C.c_int, [_p, _i, _i, _p, _i, _p]),
    "tts_token_average": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p, _p]),
}

# symbol -> (restype, argtypes); mirrors include/toucan_score.h (the corpus scorer: csrc/score.hip, stage entries in csrc/pipeline.hip)
SCORE_PROTOTYPES = {
    "tts_ctc_loss": (C.c_int, [_p, _i, _i, _p, _p, _p, _p, _p, _i, _i, _i, _p, _p]),
    "tts_score_losses": (C.c_int, [_p, _i, _p, _i, _p, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _p, _p]),
    "tts_teacher_forced": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, C.POINTER(_i), _p]),
    "tts_copy_decoder_mel": (C.c_int, [_p, _p, _i, _p]),
    # the glow loss (csrc/glow_forward.hip, stage entry in csrc/pipeline.hip)
    "tts_glow_forward_rows": (C.c_int, [_p, _i, _i, _p, _i, _p, _p, _p, _p, _p]),
    "tts_glow_nll_reduce": (C.c_int, [_p, _i, _p, _p, _p, _p, _i, C.c_double, _p, _p, _p]),
    "tts_postflow_nll": (C.c_int, [_p, _p, _i, _p, _p, _p, _p]),
}
CTC_MAX_TARGETS = 2048  # include/toucan_score.h TTS_CTC_MAX_TARGETS
GLOW_FORWARD_BLOCK_ROWS, GLOW_FORWARD_GRID_ROWS = 12, 24576  # TTS_GLOW_FORWARD_BLOCK_ROWS, _GRID_ROWS


class TtsGanConvDesc(C.Structure):
    _fields_ = [
        ("x", _p), ("w", _p), ("scale", _p), ("shift", _p), ("res", _p), ("y", _p),
        ("n", _i), ("h", _i), ("cin", _i), ("cout", _i), ("taps", _i),
        ("flags", _i),
        ("pre_slope", _f), ("res_ratio", _f), ("slope", _f),
    ]


# symbol -> (restype, argtypes); mirrors include/toucan_gan.h (the speaker-embedding GAN: csrc/gan.hip) one to one
GAN_PROTOTYPES = {
    "tts_gan_conv2d": (C.c_int, [C.POINTER(TtsGanConvDesc), _p]),
}
GAN_KC, GAN_NC = 16, 64  # include/toucan_gan.h TTS_GAN_KC, TTS_GAN_NC: weight packing
GAN_UPSAMPLE, GAN_PRE_LRELU, GAN_RESIDUAL, GAN_RES_UPSAMPLE, GAN_LRELU = 1, 2, 4, 8, 16  # TTS_GAN_* flags

# symbol -> (restype, argtypes); mirrors include/toucan_pitch.h (the pitch tracker: csrc/pitch.hip) one to one
PITCH_PROTOTYPES = {
    "tts_wave_stats": (C.c_int, [_p, _p, _p, _i, _p, _p]),
    "tts_pitch_candidates": (C.c_int, [_p, _p, _p, _p, _p, _p, _i, _i, _p, _p, _p, _p, _p, _p, _p]),
    "tts_pitch_path": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _p, _p]),
}
PITCH_CANDIDATES, PITCH_LAGS, PITCH_WINDOW = 15, 600, 1198  # include/toucan_pitch.h TTS_PITCH_CANDIDATES, _LAGS, _WINDOW
PITCH_MIN_SAMPLES, PITCH_PATH_LDS_FRAMES = 1200, 2048  # TTS_PITCH_MIN_SAMPLES, TTS_PITCH_PATH_LDS_FRAMES

# symbol -> (restype, argtypes); mirrors include/toucan_train.h (the aligner's on-line fine-tuning: csrc/train.hip) one to one
_l = C.c_int64
TRAIN_PROTOTYPES = {
    "tts_gemm_f32": (C.c_int, [_i, _p, _i, _p, _i, _p, _i, _p, _i, _i, _i, _i, _p]),
    "tts_bn_train_forward": (C.c_int, [_p, _i, _p, _p, _p, _p, _p, _p, _i, _p, _p, _i, _i, _f, _f, _p]),
    "tts_bn_train_backward": (C.c_int, [_p, _i, _p, _i, _p, _p, _p, _p, _p, _i, _p, _p, _i, _i, _p]),
    "tts_bn_eval_affine": (C.c_int, [_p, _p, _p, _p, _p, _p, _i, _f, _p]),
    "tts_lstm_train_step": (C.c_int, [_p, _i, _p, _p, _p, _p, _i, _p, _p, _i, _i, _i, _p]),
    "tts_lstm_backward_step": (C.c_int, [_p, _i, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "tts_ctc_grad": (C.c_int, [_p, _i, _i, _i, _p, _i, _i, _p, _p, _p, _p, _i, _p]),
    "tts_col_sum": (C.c_int, [_p, _i, _i, _i, _p, _p, _p]),
    "tts_sumsq": (C.c_int, [_p, _l, _p, _p, _p]),
    "tts_sgd_clip_update": (C.c_int, [_p, _p, _l, _p, _f, _f, _p]),
}
GEMM_NN, GEMM_NT, GEMM_TN = 0, 1, 2  # include/toucan_train.h TTS_GEMM_*
CTC_GRAD_MAX_TARGETS, SUMSQ_PARTIALS = 768, 256  # TTS_CTC_GRAD_MAX_TARGETS, TTS_SUMSQ_PARTIALS


class TtsResampleSpan(C.Structure):
    _fields_ = [("in_begin", _l), ("n_held", _l), ("pos0", _l), ("out_first", _l), ("out_count", _l), ("out_begin", _l)]


# symbol -> (restype, argtypes); mirrors include/toucan_resample.h (the sample-rate converter: csrc/resample.hip) one to one
RESAMPLE_PROTOTYPES = {
    "tts_resample_tile_outputs": (C.c_int, []),
    "tts_resample": (C.c_int, [_p, _p, _p, _i, _l, _i, _i, _i, _i, _p, _p]),
}
RESAMPLE_MAX_FACTOR, RESAMPLE_LDS_TABLE_BYTES = 1024, 65536  # include/toucan_resample.h TTS_RESAMPLE_MAX_FACTOR, _LDS_TABLE_BYTES

# symbol -> (restype, argtypes); mirrors include/toucan_prosody.h (per-utterance prosody scales: csrc/prosody.hip, stage entries in csrc/pipeline.hip)
PROSODY_PROTOTYPES = {
    "tts_prosody_control_v": (C.c_int, [_p, _i, _p, _p, _p, _p, _p, _i, _p, _p]),
    "tts_prosody_stats": (C.c_int, [_p, _p, _p, _p, _p, _i, _p, _p]),
    "tts_control_and_regulate_v": (C.c_int, [_p, _p, _p, _p]),
    "tts_copy_prosody_stats": (C.c_int, [_p, _p, _p, _p]),
}
PROSODY_SCALES, PROSODY_STATS = 4, 8  # include/toucan_prosody.h TTS_PROSODY_SCALES, TTS_PROSODY_STATS

# symbol -> (restype, argtypes); mirrors include/toucan_prosody_curves.h (per-phoneme prosody curves: csrc/prosody.hip, stage entries in csrc/pipeline.hip)
CURVE_PROTOTYPES = {
    "tts_prosody_control_c": (C.c_int, [_p, _i, _p, _p, _p, _p, _p, _i, _p, _p, _p]),
    "tts_control_and_regulate_c": (C.c_int, [_p, _p, _p, _p, _i, _p, _p]),
    "tts_copy_prosody_span_stats": (C.c_int, [_p, _p, _p, _p]),
}
PROSODY_CURVE_COLUMNS = 5  # include/toucan_prosody_curves.h TTS_PROSODY_CURVE_COLUMNS

# symbol -> (restype, argtypes); mirrors include/toucan_prosody_fit.h (the time budget: csrc/prosody.hip, stage entries in csrc/pipeline.hip)
FIT_PROTOTYPES = {
    "tts_prosody_fit": (C.c_int, [_p, _i, _p, _p, _p, _i, _p, _p, _p, _p, _i, _p, _p, _p, _p, _p, _p, _p, _p]),
    "tts_prosody_fit_apply": (C.c_int, [_p, _p, _i, _p]),
    "tts_control_and_regulate_t": (C.c_int, [_p, _p, _p, _p, _i, _p, _i, _p, _p]),
    "tts_copy_prosody_fit": (C.c_int, [_p, _p, _p, _p, _p]),
}
FIT_UTT_DURATION, FIT_UTT_PAUSE, FIT_SPAN = 0, 1, 2  # include/toucan_prosody_fit.h TTS_FIT_UTT_DURATION, _UTT_PAUSE, _SPAN
FIT_SPEC, FIT_N_COLUMNS, FIT_MAX_TARGET, FIT_MAX_BOUND = 4, 8, 1 << 24, 64  # TTS_FIT_SPEC, TTS_FIT_COLUMNS, TTS_FIT_MAX_TARGET, TTS_FIT_MAX_BOUND


class TtsDtwPair(C.Structure):
    _fields_ = [("begin_a", _i), ("frames_a", _i), ("begin_b", _i), ("frames_b", _i), ("scratch_off", _l), ("path_begin", _l)]


# symbol -> (restype, argtypes); mirrors include/toucan_compare.h (cepstra, DTW and the sums along its path: csrc/compare.hip) one to one
COMPARE_PROTOTYPES = {
    "tts_dtw_max_frames": (C.c_int, []),
    "tts_mel_cepstra": (C.c_int, [_p, _i, _i, _p, _i, _p, _i, _p, _p]),
    "tts_dtw": (C.c_int, [_p, _i, _p, _i, _i, C.POINTER(TtsDtwPair), _p, _i, _p, _l, _i, _p, _l, _p, _p, _p]),
    "tts_dtw_path_sums": (C.c_int, [_p, _i, _p, _i, _i, C.POINTER(TtsDtwPair), _p, _i, _p, _l, _p, _p, _p, _p, _p]),
}
COMPARE_MELS, COMPARE_MAX_CEP = 80, 32  # include/toucan_compare.h TTS_COMPARE_MELS, TTS_COMPARE_MAX_CEP
DTW_MAX_FRAMES, DTW_LDS_BP_BYTES, DTW_N_SUMS = 4096, 40960, 12  # TTS_DTW_MAX_FRAMES, TTS_DTW_LDS_BP_BYTES, TTS_DTW_N_SUMS
# the columns of tts_dtw_path_sums, in the order of the header's TTS_DTW_SUM_* indices
DTW_SUM_COLUMNS = ("mcd", "diag", "vv", "sq_hz", "sq_cents", "x", "y", "xx", "yy", "xy", "gross", "vuv")

class TtsPronUtt(C.Structure):
    _fields_ = [("frame_begin", _i), ("n_frames", _i), ("ref_begin", _i), ("n_ref", _i), ("scratch_off", _l)]


# symbol -> (restype, argtypes); mirrors include/toucan_pronunciation.h (CTC decoders, edit distance, posteriors over the forced alignment: csrc/pronunciation.hip) one to one
PRONUNCIATION_PROTOTYPES = {
    "tts_ctc_best_path": (C.c_int, [_p, _i, _i, _i, _i, _p, C.POINTER(TtsPronUtt), _p, _i, _p, _p, _p, _p, _p, _p]),
    "tts_ctc_beam_search": (C.c_int, [_p, _i, _i, _i, _i, _p, C.POINTER(TtsPronUtt), _p, _i, _i, _p, _l, _p, _p, _p, _p]),
    "tts_edit_distance": (C.c_int, [_p, _i, _p, _i, _p, C.POINTER(TtsPronUtt), _p, _i, _p, _l, _i, _p, _p, _p, _p]),
    "tts_phone_posteriors": (C.c_int, [_p, _i, _i, _i, _p, _p, _i, C.POINTER(TtsPronUtt), _p, _i, _p, _p]),
}
# include/toucan_pronunciation.h TTS_PRON_MAX_SYMBOLS, TTS_BEAM_MAX, TTS_CTC_SCAN_BLOCK, TTS_EDIT_MAX_REF, TTS_EDIT_MAX_HYP, TTS_EDIT_LDS_BP_BYTES, TTS_PHONE_COLUMNS
PRON_MAX_SYMBOLS, BEAM_MAX, CTC_SCAN_BLOCK, EDIT_MAX_REF, EDIT_MAX_HYP, EDIT_LDS_BP_BYTES, PHONE_COLUMNS = 256, 32, 256, 2048, 4096, 28672, 4

# symbol -> (restype, argtypes); mirrors include/toucan_loudness.h (BS.1770 loudness and the gain to a target: csrc/loudness.hip) one to one
LOUDNESS_PROTOTYPES = {
    "tts_loudness_tile_segments": (C.c_int, []),
    "tts_kweight_energy": (C.c_int, [_p, _l, _p, _p, _i, _i, _p, _l, _p, _p, _p, _p]),
    "tts_loudness_gate": (C.c_int, [_p, _p, _l, _p, _i, _i, _l, C.c_double, C.c_double, _p, _p]),
    "tts_apply_gain": (C.c_int, [_p, _l, _p, _p, _i, _l, _p, _p, _p]),
}
# include/toucan_loudness.h TTS_LOUDNESS_MIN_RATE, _MAX_RATE, _COLUMNS, _TABLE_DOUBLES
LOUDNESS_MIN_RATE, LOUDNESS_MAX_RATE, LOUDNESS_N_COLUMNS, LOUDNESS_TABLE_DOUBLES = 8000, 192000, 8, 24

# symbol -> (restype, argtypes); mirrors include/toucan_activity.h (ITU-T P.56 active speech level, runs of speech: csrc/activity.hip) one to one
ACTIVITY_PROTOTYPES = {
    "tts_activity_tile_segments": (C.c_int, []),
    "tts_activity_envelope": (C.c_int, [_p, _l, _p, _p, _i, _i, _p, _l, _p, _p, _p, _p, _p]),
    "tts_activity_level": (C.c_int, [_p, _p, _p, _l, _p, _i, _i, _l, C.c_double, C.c_double, _p, _p, _p, _p]),
    "tts_activity_runs": (C.c_int, [_p, _l, _p, _p, _i, _i, _p, _l, _p, _p, _i, _p, _p, _p, _p]),
}
# include/toucan_activity.h TTS_ACTIVITY_MIN_RATE, _MAX_RATE, _COLUMNS, _THRESHOLDS, _COUNTS, _TABLE_DOUBLES
ACTIVITY_MIN_RATE, ACTIVITY_MAX_RATE, ACTIVITY_N_COLUMNS, ACTIVITY_THRESHOLDS, ACTIVITY_COUNTS, ACTIVITY_TABLE_DOUBLES = 8000, 192000, 8, 15, 16, 6

# symbol -> (restype, argtypes); mirrors include/toucan_truepeak.h (true peak, loudness range, the gain under a true-peak ceiling: csrc/truepeak.hip) one to one
TRUEPEAK_PROTOTYPES = {
    "tts_truepeak_tile_samples": (C.c_int, []),
    "tts_true_peak": (C.c_int, [_p, _l, _p, _p, _i, _l, _p, _i, _p, _p, _p]),
    "tts_loudness_range": (C.c_int, [_p, _p, _p, _l, _p, _i, _i, _l, _p, _p, _p]),
    "tts_truepeak_gain": (C.c_int, [_p, _l, _p, _p, _i, _p, _i, _p, C.c_double, _p, _p, _p, _p]),
    "tts_limit_true_peak": (C.c_int, [_p, _l, _p, _p, _i, _l, _i, _p, _i, _p, C.c_double, C.c_double, C.c_double, _p, _p, _p, _p, _p, _p]),
}
# include/toucan_truepeak.h TTS_TRUEPEAK_TAPS, _HALF_WIDTH, _MAX_STEPS, _TILED_ROUNDS, _SHORT_TERM_SEGMENTS, TTS_DELIVERY_COLUMNS, TTS_LIMITER_COLUMNS
TRUEPEAK_TAPS, TRUEPEAK_HALF_WIDTH, TRUEPEAK_MAX_STEPS, TRUEPEAK_TILED_ROUNDS, TRUEPEAK_SHORT_TERM_SEGMENTS, DELIVERY_N_COLUMNS, LIMITER_N_COLUMNS = 15, 7, 128, 3, 30, 12, 8

# symbol -> (restype, argtypes); mirrors include/toucan_fidelity.h (reflection framing, spectral distances of a pair of waveforms: csrc/fidelity.hip) one to one
FIDELITY_PROTOTYPES = {
    "tts_spectral_frames_per_group": (C.c_int, []),
    "tts_spectral_reduce_sweep": (C.c_int, []),
    "tts_frame_reflect": (C.c_int, [_p, _l, _p, _p, _i, _l, _i, _p, _p, _l, _p, _p]),
    "tts_spectral_distance": (C.c_int, [_p, _l, _i, _l, _p, _p, _i, _l, _p, _p, _i, _p, _i, _p, _p]),
    "tts_spectral_reduce": (C.c_int, [_p, _p, _i, _l, _p, _p]),
}
# include/toucan_fidelity.h TTS_FIDELITY_SUMS, _MAX_BINS, _MAX_BANDS, _MAX_HOP
FIDELITY_SUMS, FIDELITY_MAX_BINS, FIDELITY_MAX_BANDS, FIDELITY_MAX_HOP = 4, 2049, 256, 4096

# symbol -> (restype, argtypes); mirrors include/toucan_intelligibility.h (STOI and ESTOI of time-aligned pairs: csrc/intelligibility.hip) one to one
INTELLIGIBILITY_PROTOTYPES = {
    "tts_stoi_select_sweep": (C.c_int, []),
    "tts_stoi_segments_per_group": (C.c_int, []),
    "tts_stoi_frame_energy": (C.c_int, [_p, _l, _p, _p, _i, _p, _l, _p, _p]),
    "tts_stoi_select": (C.c_int, [_p, _p, _p, _i, _l, _l, _p, _p, _p]),
    "tts_stoi_gather": (C.c_int, [_p, _l, _p, _p, _i, _p, _l, _p, _p, _p, _p, _l, _p, _p]),
    "tts_stoi_bands": (C.c_int, [_p, _l, _l, _p, _p]),
    "tts_stoi_segments": (C.c_int, [_p, _l, _p, _p, _p, _p, _i, _l, _p, _p]),
    "tts_stoi_reduce": (C.c_int, [_p, _p, _i, _l, _p, _p]),
}
# include/toucan_intelligibility.h TTS_STOI_RATE, _FRAME, _HOP, _BINS, _BANDS, _SEGMENT, _MAX_FRAMES, _BAND_EDGES
STOI_RATE, STOI_FRAME, STOI_HOP, STOI_BINS, STOI_BANDS, STOI_SEGMENT, STOI_MAX_FRAMES = 10000, 256, 128, 257, 15, 30, 8388608
STOI_BAND_EDGES = (7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219)

# symbol -> (restype, argtypes); mirrors include/toucan_prominence.h (word prominence and boundary strength from the wavelet transform of prosodic tracks: csrc/prominence.hip) one to one
_d = C.c_double
PROMINENCE_PROTOTYPES = {
    "tts_prominence_max_frames": (C.c_int, []),
    "tts_prominence_channels": (C.c_int, [_p, _p, _l, _p, _p, _i, _p, _p, _l, _p, _p]),
    "tts_prominence_cwt": (C.c_int, [_p, _l, _p, _p, _i, _p, _p, _p]),
    "tts_prominence_units": (C.c_int, [_p, _l, _p, _p, _i, _p, _p, _l, _d, _d, _d, _i, _i, _p, _p, _p]),
}
# include/toucan_prominence.h TTS_PROMINENCE_MAX_FRAMES, _CHANNELS, _SCALES, _MAX_TAPS, _TABLE_LD, _COLUMNS, _UTT_COLUMNS, _TILE
PROMINENCE_MAX_FRAMES, PROMINENCE_CHANNELS, PROMINENCE_SCALES, PROMINENCE_MAX_TAPS, PROMINENCE_TABLE_LD = 65536, 3, 6, 1025, 1026
PROMINENCE_N_COLUMNS, PROMINENCE_UTT_COLUMNS, PROMINENCE_TILE = 8, 6, 256

_LIB = None
ABI_VERSION = 15  # include/toucan_tts.h TTS_ABI_VERSION: struct layouts and prototypes mirrored below


class ToucanHipError(RuntimeError):
    pass


def lib():
    """Load libtoucan_hip.so and bind every symbol of the ABI; raise loudly if anything is missing."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ToucanHipError(
            f"{LIB_PATH} not found: the HIP extension is mandatory (no CPU fallback). "
            f"Build it with `python -c 'import __graft_entry__ as g; g.build()'`.")
    # PyTorch-ROCm ships its own libamdhip64; load it FIRST so that libtoucan_hip.so binds to the same HIP
    # runtime (same soname) - two runtimes in one process cannot share streams or device pointers.
    import torch  # noqa: F401
    handle = C.CDLL(LIB_PATH)
    _assert_single_hip_runtime()
    for name, (res, args) in list(PROTOTYPES.items()) + list(ALIGN_PROTOTYPES.items()) + list(SCORE_PROTOTYPES.items()) + \
            list(GAN_PROTOTYPES.items()) + list(PITCH_PROTOTYPES.items()) + list(TRAIN_PROTOTYPES.items()) + list(RESAMPLE_PROTOTYPES.items()) + \
            list(PROSODY_PROTOTYPES.items()) + list(CURVE_PROTOTYPES.items()) + list(COMPARE_PROTOTYPES.items()) + \
            list(PRONUNCIATION_PROTOTYPES.items()) + list(LOUDNESS_PROTOTYPES.items()) + list(ACTIVITY_PROTOTYPES.items()) + \
            list(TRUEPEAK_PROTOTYPES.items()) + list(FIDELITY_PROTOTYPES.items()) + list(FIT_PROTOTYPES.items()) + \
            list(INTELLIGIBILITY_PROTOTYPES.items()) + list(PROMINENCE_PROTOTYPES.items()):
        try:
            fn = getattr(handle, name)
        except AttributeError as e:
            raise ToucanHipError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    got = handle.tts_abi_version()
    if got != ABI_VERSION:
        raise ToucanHipError(f"{LIB_PATH} reports ABI version {got}, this binding was written for {ABI_VERSION}: rebuild the "
                             f"library (python -c 'import __graft_entry__ as g; g.build()')")
    _LIB = handle
    return handle


def _assert_single_hip_runtime():
    try:
        with open("/proc/self/maps") as f:
            paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    except OSError:
        return
    if len(paths) > 1:
        raise ToucanHipError(f"two HIP runtimes are mapped ({sorted(paths)}); import torch before loading libtoucan_hip.so")


CALLS = 0  # ABI calls checked so far (bench.py reports the calls of one pass)


def check(rc, what=""):
    global CALLS
    CALLS += 1
    if rc != 0:
        msg = lib().tts_last_error().decode("utf-8", "replace")
        raise ToucanHipError(f"{what} failed with code {rc}: {msg}")
