"""ctypes binding of libstylish_hip.so (include/stylish_hip.h).

The product path has no CPU fallback: if the HIP library is missing or fails to load this module raises,
and every operator raises RuntimeError on a non-zero status with the library's error text.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# STTS_LIB: another build of the library next to the product one (diagnostic builds: STTS_BUILD_TAG=_wntrace STTS_HIPCC_FLAGS=-DSTTS_WN_TRACE ...)
LIB_PATH = os.path.abspath(os.environ["STTS_LIB"]) if os.environ.get("STTS_LIB") else os.path.join(_HERE, "libstylish_hip.so")


class ModelDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "n_fft", "win_length", "hop_length", "sample_rate",
        "style_dim", "inter_dim",
        "dec_hidden", "dec_residual",
        "gen_input", "gen_hidden", "gen_inter", "gen_io_kernel",
        "tokens", "te_hidden", "te_filter", "te_heads", "te_layers", "te_kernel",
        "style_layers",
        "dur_layers", "dur_classes", "dur_max",
        "pe_inter",
    )]


class CfmDims(C.Structure):
    """include/stylish_hip.h: stts_cfm_dims (the constructor keywords of the reference's CfmMelDecoder)."""
    _fields_ = [(n, C.c_int32) for n in ("feat_dim", "asr_dim", "spk_dim", "hidden_dim", "emb_dim", "depth", "enc_blocks", "dec_blocks",
                                         "prev_depth", "post_depth", "head_dim")]


def dims_from_config(cfg) -> ModelDims:
    g, te, du = cfg.generator, cfg.text_encoder, cfg.duration_predictor
    return ModelDims(
        cfg.n_fft, cfg.win_length, cfg.hop_length, cfg.sample_rate,
        cfg.style_dim, cfg.inter_dim,
        cfg.decoder.hidden_dim, cfg.decoder.residual_dim,
        g.input_dim, g.hidden_dim, g.conv_intermediate_dim, g.io_conv_kernel_size,
        te.tokens, te.hidden_dim, te.filter_channels, te.heads, te.layers, te.kernel_size,
        cfg.style_encoder.layers,
        du.n_layer, du.duration_classes, du.max_duration,
        cfg.pitch_energy_predictor.inter_dim,
    )


_P = C.c_void_p
_I = C.c_int
_SZ = C.c_size_t
_I64 = C.c_int64


class ConvEpiSeg(C.Structure):
    """include/stylish_hip.h: stts_conv_epi_seg (test surface)."""
    _fields_ = [("x", _P), ("w_host", _P), ("x_elems", _I64), ("ldx", C.c_int32), ("cin", C.c_int32), ("k", C.c_int32), ("dil", C.c_int32)]


class ConvEpiArgs(C.Structure):
    """include/stylish_hip.h: stts_conv_epi_args (test surface)."""
    _fields_ = ([("seg_off_host", _P), ("seg_off_dev", _P), ("seg", ConvEpiSeg * 2)]
                + [(n, _P) for n in ("bias_host", "r", "y", "y16", "sumsq", "stat")]
                + [(n, _I64) for n in ("r_elems", "y_elems", "y16_elems", "sumsq_elems", "stat_elems")]
                + [(n, C.c_int32) for n in ("n_utt", "capacity", "nseg", "cout", "act")]
                + [("alpha", C.c_float)]
                + [(n, C.c_int32) for n in ("ldr", "rcol0", "ldy", "ycol0", "ldy16", "ycol16", "ld_ss", "ss_stride", "ld_stat", "stat_nchunk",
                                            "force_tile", "tune", "precision")])

def _fields(*groups):
    """(type, "a b c") groups -> ctypes _fields_, in order."""
    return [(n, t) for t, names in groups for n in names.split()]


_I32, _F = C.c_int32, C.c_float


class AdainArgs(C.Structure):
    """include/stylish_hip.h: stts_adain_args (test surface)."""
    _fields_ = _fields((_P, "seg_off_host seg_off_dev x part partial bias r gb snake aff y"),
                       (_I64, "x_elems part_elems partial_elems bias_elems r_elems gb_elems snake_elems aff_elems y_elems"),
                       (_I32, "n_utt producer consumer C ldx ldp nchunk ksplit slice_rows ld_part split_n split_act ldr rcol0"), (_F, "split_alpha"),
                       (_I32, "ld_gb gcol0 ld_aff ldy rb act out16"))


class AdainChainBlock(C.Structure):
    """include/stylish_hip.h: stts_adain_chain_block (test surface)."""
    _fields_ = _fields((C.c_char_p, "prefix"), (_P, "y y16"), (_I64, "y_elems y16_elems"), (_I32, "cin cout ldy ldy16"))


class AdainChainArgs(C.Structure):
    """include/stylish_hip.h: stts_adain_chain_args (test surface)."""
    _fields_ = (_fields((_P, "seg_off_host seg_off_dev x style ws plan_out"), (_I64, "x_elems style_elems ws_bytes"), (_I32, "n_utt nblocks ldx"),
                        (_I32, "fold_rows fold16_rows rows16 sc_side_min_rows affine_serial no_wino_conv2sc no_stat_fuse no_wino_stats bridge"),
                        (_I32, "offer_wino offer_stats offer_rows16 offer_side defer force_tile")) + [("blocks", AdainChainBlock * 2)])


class WinoStatArgs(C.Structure):
    """include/stylish_hip.h: stts_wino_stat_args (test surface)."""
    _fields_ = _fields((_P, "seg_off_host seg_off_dev x w_host bias_host y stat"), (_I64, "x_elems y_elems stat_elems"),
                       (_I32, "n_utt ldx cin cout k act ldy ld_stat stat_nchunk precision"))


class LnOutArgs(C.Structure):
    """include/stylish_hip.h: stts_ln_out (test surface)."""
    _fields_ = _fields((_P, "y g b"), (_I64, "y_elems g_elems b_elems"), (_I32, "ldy ycol0 ld_g gcol0 prec16"))


class RowLayerNormArgs(C.Structure):
    """include/stylish_hip.h: stts_row_layernorm_args (test surface)."""
    _fields_ = (_fields((_P, "seg_off_host seg_off_dev x partial bias r"), (_I64, "x_elems partial_elems bias_elems r_elems")) + [("out", LnOutArgs * 2)]
                + _fields((_I32, "n_utt n_rows n_rows_real C ldx adaptive nout act"), (_F, "eps"), (_I32, "ksplit slice_rows ld_part in_act ldr rcol0"), (_F, "in_alpha")))


class DwconvArgs(C.Structure):
    """include/stylish_hip.h: stts_dwconv_args (test surface)."""
    _fields_ = _fields((_P, "seg_off_host seg_off_dev x w_host bias_host style y"), (_I64, "x_elems style_elems y_elems"),
                       (_I32, "n_utt form C K act ldx ldy ld_style gcol0 prec16"))


class GrnArgs(C.Structure):
    """include/stylish_hip.h: stts_grn_args (test surface)."""
    _fields_ = _fields((_P, "seg_off_host seg_off_dev part gamma w gx xaff wu"), (_I64, "part_elems gamma_elems w_elems gx_elems xaff_elems wu_elems"),
                       (_I32, "n_utt mode C ld_ss ss_stride ld_gx ld_xaff npad kc prec"))


class Conv2dArgs(C.Structure):
    """include/stylish_hip.h: stts_conv2d_args (test surface)."""
    _fields_ = (_fields((_P, "w_host bias_host off_in_host off_in_dev off_out_host off_out_dev x0 x1 r y"), (_I64, "x0_elems x1_elems r_elems y_elems"))
                + [("dt", _I32 * 25), ("df", _I32 * 25)]
                + _fields((_I32, "ntap cout cin0 cin1 ld0 ld1 npad lrelu chunk sliced n_utt sh Fin F up pt pf act"), (_F, "div"), (_I32, "ldy")))


class CfmElemArgs(C.Structure):
    """include/stylish_hip.h: stts_cfm_elem_args (test surface)."""
    _fields_ = _fields((_P, "seg_off_host seg_off_dev x t ada y"), (_I64, "x_elems t_elems ada_elems y_elems n"), (_I32, "n_utt kind C"))


class RmsAdalnArgs(C.Structure):
    """include/stylish_hip.h: stts_rms_adaln_args (test surface)."""
    _fields_ = _fields((_P, "seg_off_host seg_off_dev x w ada y t ada_prev xout"), (_I64, "x_elems w_elems ada_elems y_elems t_elems ada_prev_elems xout_elems"),
                       (_I32, "n_utt C ldx ldy"))


class RopeArgs(C.Structure):
    """include/stylish_hip.h: stts_rope_args (test surface)."""
    _fields_ = _fields((_P, "seg_off_host seg_off_dev x freq"), (_I64, "x_elems freq_elems"), (_I32, "n_utt kind ldx col0 col1 heads kc d"))


class CfmSmallArgs(C.Structure):
    """include/stylish_hip.h: stts_cfm_small_args (test surface)."""
    _fields_ = _fields((_P, "x w b y"), (_I64, "x_elems w_elems b_elems y_elems"), (_I32, "kind n_rows N K act ldx ldy"))


class CfmSourceArgs(C.Structure):
    """include/stylish_hip.h: stts_cfm_source_args (test surface)."""
    _fields_ = _fields((_P, "seg_off_host seg_off_dev curve_off_host curve_off_dev f0 ncurve t noise har"), (_I64, "f0_elems ncurve_elems t_elems noise_elems har_elems"),
                       (_I32, "n_utt ldh"), (_F, "merge_w"))


class GlueArgs(C.Structure):
    """include/stylish_hip.h: stts_glue_args (test surface)."""
    _fields_ = (_fields((_P, "seg_off_host seg_off_dev tok_off_host tok_off_dev x x2 x3 w_host b_host tokens dur y y2 y3 iy iy2 err"),
                        (_I64, "x_elems x2_elems x3_elems tokens_elems dur_elems y_elems y2_elems y3_elems iy_elems iy2_elems"),
                        (_I32, "n_utt kind n_rows C K J ldx ldy ld2 col0 rep c_hidden c_res"))
                + [("wf", _F * 3), ("bf", _F), ("wn", _F * 3), ("bn", _F)])


class ChanConvArgs(C.Structure):
    """include/stylish_hip.h: stts_chan_conv_args (test surface)."""
    _fields_ = _fields((_P, "seg_off_host seg_off_dev x0 x1 w0 w1 y0 y1"), (_I64, "x0_elems x1_elems w0_elems w1_elems y0_elems y1_elems"),
                       (_I32, "n_utt prec16 nsets ntaps C ldx ldy ycol"), (_F, "bias0 bias1"))


# name -> (restype, argtypes); mirrors include/stylish_hip.h one to one
SIGNATURES = {
    "stts_last_error": (C.c_char_p, []),
    "stts_version": (_I, []),
    "stts_ctx_create": (_I, [C.POINTER(ModelDims), _I, C.POINTER(_P)]),
    "stts_ctx_destroy": (None, [_P]),
    "stts_load_weight": (_I, [_P, C.c_char_p, _P, C.POINTER(_I64), _I]),
    "stts_finalize_weights": (_I, [_P, _I]),
    "stts_check_status": (_I, [_P, _P]),
    "stts_frame_workspace_bytes": (_SZ, [_P, _I64, _I, _I]),
    "stts_har_ld": (_I, [_P]),
    "stts_decoder_forward": (_I, [_P, _P, _I, _P, _P, _P, _I, _P, _P, _P, _P, _I, _P, _SZ]),
    "stts_prior_flow_forward": (_I, [_P, _P, _I, _P, _P, _P, _I, _P, _P, _P, _I, _P, _P, _P, _SZ]),
    "stts_harmonic_stft": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _P, _SZ]),
    "stts_vocoder_forward": (_I, [_P, _P, _I, _P, _P, _P, _I, _P, _P, _P, _I, _P, _P, _P, _I, _P, _SZ]),
    "stts_frame_path": (_I, [_P, _P, _I, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _SZ, _I]),
    "stts_posterior_forward": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _SZ, _I]),
    "stts_posterior_workspace_bytes": (_SZ, [_P, _I64, _I, _I]),
    "stts_flow_stats_forward": (_I, [_P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _SZ, _I]),
    "stts_flow_stats_workspace_bytes": (_SZ, [_P, _I64, _I, _I]),
    "stts_prior_stats_forward": (_I, [_P, _P, _I, _P, _P, _P, _I, _P, _P, _P, _P, _P, _SZ, _I]),
    "stts_val_kl_sums": (_I, [_P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _I, _I, _P, _P, _SZ]),
    "stts_frame_offsets": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _P]),
    "stts_phoneme_workspace_bytes": (_SZ, [_P, _I64, _I64, _I, _I, _I]),
    "stts_text_encoder_forward": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _I, _P, _P, _SZ]),
    "stts_text_style_forward": (_I, [_P, _P, _I, _I, _P, _P, _P, _I, _P, _P, _SZ]),
    "stts_duration_forward": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _SZ]),
    "stts_pitch_energy_forward": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _SZ, _I]),
    "stts_duration_decode": (_I, [_P, _P, _I, _I, _P]),
    "stts_duration_to_alignment": (_I, [_P, _P, _I, _I, _P]),
    "stts_length_regulate": (_I, [_P, _P, _I, _P, _P, _P, _I64, _I, _P, _I, _I, _P, _I, _P]),
    "stts_set_precision": (_I, [_P, _I]),
    "stts_upsample4": (_I, [_P, _P, _I, _P, _P, _P, _P, _P]),
    "stts_euler_step": (_I, [_P, _P, _P, C.c_float, C.c_int64]),
    "stts_hubert_workspace_bytes": (_SZ, [_P, C.c_int64, _I, _I]),
    "stts_speaker_style": (_I, [_P, _P, _I, _P, _I, _P, _P, _P, _SZ]),
    "stts_hubert_encoder_forward": (_I, [_P, _P, _I, _P, _P, _P, _I, _P, _I, _P, _SZ]),
    "stts_hubert_pitch_energy_forward": (_I, [_P, _P, _I, _P, _P, _P, _I, _P, _P, _P, _P, _P, _SZ]),
    "stts_mel_style_workspace_bytes": (_SZ, [_P, _I, _I64, _I]),
    "stts_mel_style_forward": (_I, [_P, _P, _I, _I, _P, _P, _P, _I, _P, _P, _SZ]),
    "stts_mel_style_forward_taps": (_I, [_P, _P, _I, _I, _P, _P, _P, _I, _P, _P, _P, _SZ]),
    "stts_cfm_pitch_workspace_bytes": (_SZ, [_P, _I64, _I]),
    "stts_cfm_pitch_forward": (_I, [_P, _P, _I, _P, _P, _P, _I, _P, _P, _P, C.c_float, C.c_float, _P, _P, _SZ]),
    "stts_cfm_pitch_forward_taps": (_I, [_P, _P, _I, _P, _P, _P, _I, _P, _P, _P, C.c_float, C.c_float, _P, _P, _P, _SZ]),
    "stts_ssl_finalize": (_I, [_P, _P]),
    "stts_ssl_frames": (_I64, [_P, _I64]),
    "stts_ssl_workspace_bytes": (_SZ, [_P, _I, _P]),
    "stts_ssl_forward": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _P, _SZ]),
    "stts_ssl_forward_taps": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _SZ]),
    "stts_ssl_tap_rows": (_I64, [_P, _I, _P]),
    "stts_wavlm_finalize": (_I, [_P, _P]),
    "stts_wavlm_workspace_bytes": (_SZ, [_P, _I, _P, _I]),
    "stts_wavlm_forward_states": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _P, _SZ]),
    "stts_wavlm_l1_sums": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _P, _SZ]),
    "stts_wavlm_bucket_table": (_I, [_P, _I, _P]),
    "stts_rmvpe_finalize": (_I, [_P, _P]),
    "stts_rmvpe_workspace_bytes": (_SZ, [_P, _I, _P]),
    "stts_rmvpe_forward": (_I, [_P, _P, _I, _P, _P, _P, _I, C.c_float, _P, _P, _P, _SZ]),
    "stts_rmvpe_forward_taps": (_I, [_P, _P, _I, _P, _P, _P, _I, C.c_float, _P, _P, _P, _P, _SZ]),
    "stts_rmvpe_tap_floats": (_I64, [_P, _I, _P]),
    "stts_rmvpe_mel": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "stts_rmvpe_decode": (_I, [_P, _P, _I64, _P, _I, C.c_float, _P]),
    "stts_rmvpe_decode_at": (_I, [_P, _P, _I64, _P, _I, _P, C.c_float, _P]),
    "stts_rmvpe_viterbi_workspace_bytes": (_SZ, [_I, _P]),
    "stts_rmvpe_viterbi": (_I, [_P, _P, _I, _P, _P, _P, _I, _P, C.c_double, C.c_double, C.c_float, _P, _P, _P, _P, _SZ]),
    "stts_rmvpe_resample": (_I, [_P, _P, _I, _P, _P, _P, _P, _P]),
    "stts_aligner_finalize": (_I, [_P, _P]),
    "stts_aligner_workspace_bytes": (_SZ, [_P, _I, _P]),
    "stts_aligner_forward": (_I, [_P, _P, _I, _P, _P, _P, _I, _P, _I, _P, _SZ]),
    "stts_aligner_forward_taps": (_I, [_P, _P, _I, _P, _P, _P, _I, _P, _I, _P, _P, _SZ]),
    "stts_aligner_tap_floats": (_I64, [_P, _I, _P]),
    "stts_ctc_align_workspace_bytes": (_SZ, [_I, _P, _P]),
    "stts_ctc_align": (_I, [_P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _SZ]),
    "stts_ctc_nll": (_I, [_P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, C.c_double, _P]),
    "stts_ctc_confidence_sums": (_I, [_P, _I, _P, _P, _P, _P]),
    "stts_ctc_prior_sums_workspace_bytes": (_SZ, [_I, _P, _I]),
    "stts_ctc_prior_sums": (_I, [_P, _I, _P, _P, _P, _I, _I, _P, _P, _SZ]),
    "stts_log_mel_forward": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, C.c_double, C.c_double, _P, _I, _P, _P]),
    "stts_log_mel_stats": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "stts_log_mel_filters": (_I, [_I, _I, _I, _P, _P]),
    "stts_val_sizes": (_I, [_I, _P, _I, _I, _P]),
    "stts_multi_spectrogram_forward": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _P, _P, _I]),
    "stts_val_mel_sums": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "stts_val_magphase_sums": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "stts_val_smooth_l1_sums": (_I, [_P, _P, _I, _P, _P, _P, _P, _P]),
    "stts_val_diff_sums": (_I, [_P, _P, _I, _P, _P, _P, _P, _I, _P]),
    "stts_val_duration_sums": (_I, [_P, _P, _I, _P, _P, _P, _I, _I, _P, _P, _P]),
    "stts_resample_geometry": (_I, [_I, _I, _I, C.c_double, _P, _P, _P, _P]),
    "stts_resample_out_length": (_I64, [_I64, _I, _I]),
    "stts_resample_tile": (_I, [_I, _I]),
    "stts_resample_forward": (_I, [_P, _P, _I, _I, _I, C.c_double, _I, C.c_double, _I, _P, _P, _P, _P, _P, _P]),
    "stts_cfm_finalize": (_I, [_P, _P]),
    "stts_cfm_workspace_bytes": (_SZ, [_P, _I64, _I]),
    "stts_cfm_estimator": (_I, [_P, _P, _I, _P, _P, _P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _SZ]),
    "stts_to_time_major": (_I, [_P, _P, _I, _I, _I, _P, _I]),
    "stts_to_channel_major": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "stts_conv_stft_transform": (_I, [_P, _P, _I, _P, _P, _P, _I, _P, _P, _P, _I]),
    "stts_conv_stft_inverse": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _I, _I, _P, _P, _SZ]),
    "stts_profile_begin": (_I, []),
    "stts_profile_end": (_I, [_P, C.POINTER(_I), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "stts_profile_report": (_I, [_P, C.c_char_p, _SZ]),
    "stts_op_mrf_block": (_I, [_P, _P, C.c_char_p, _I, _P, _P, _P, _I, _I, _I, _P, _P, _I, _P, _SZ]),
}
# the test surface (include/stylish_hip.h under STTS_TEST_OPS): present only in a library built with -DSTTS_TEST_OPS
TEST_SIGNATURES = {
    "stts_bench_gemm": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_double), _I]),
    "stts_op_conv1d": (_I, [_P, _I, _P, _P, _P, _I, _I, _P, _P, _I, _I, _I, _I, _P, _I, _I, _I]),
    "stts_op_conv1d_x3": (_I, [_P, _I, _P, _P, _P, _I, _I, _P, _I, _I, _P, _P, _I, _I, _I, _P, _I, C.c_float, _I, _P, _I, _I, _I]),
    "stts_op_conv1d_epi": (_I, [_P, C.POINTER(ConvEpiArgs)]),
    "stts_op_adain": (_I, [_P, C.POINTER(AdainArgs)]),
    "stts_op_wino_stat": (_I, [_P, C.POINTER(WinoStatArgs)]),
    "stts_op_row_layernorm": (_I, [_P, C.POINTER(RowLayerNormArgs)]),
    "stts_op_dwconv": (_I, [_P, C.POINTER(DwconvArgs)]),
    "stts_op_grn": (_I, [_P, C.POINTER(GrnArgs)]),
    "stts_op_conv2d": (_I, [_P, C.POINTER(Conv2dArgs)]),
    "stts_op_cfm_elem": (_I, [_P, C.POINTER(CfmElemArgs)]),
    "stts_op_rms_adaln": (_I, [_P, C.POINTER(RmsAdalnArgs)]),
    "stts_op_rope": (_I, [_P, C.POINTER(RopeArgs)]),
    "stts_op_cfm_small": (_I, [_P, C.POINTER(CfmSmallArgs)]),
    "stts_op_cfm_source": (_I, [_P, C.POINTER(CfmSourceArgs)]),
    "stts_op_glue": (_I, [_P, C.POINTER(GlueArgs)]),
    "stts_op_chan_conv": (_I, [_P, C.POINTER(ChanConvArgs)]),
    "stts_op_adain_block": (_I, [_P, _P, C.c_char_p, _I, _P, _P, _P, _I, _I, _I, _P, _P, _I, _P, _SZ]),
    "stts_op_adain_chain": (_I, [_P, _P, C.POINTER(AdainChainArgs)]),
    "stts_op_attention": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _I, _I]),
    "stts_op_wavlm_l1": (_I, [_P, _I, _P, _P, _P, _P, _I, _I, _P, _P, _P]),
    "stts_op_stft_geom": (_I, [_P, _I, _P, _P, _I, _I, _I, _P, _P, _P, _I, _I]),
    "stts_op_istft_geom": (_I, [_P, _I, _P, _P, _I, _I, _I, _P, _P, _I, _P, _I]),
    "stts_op_posterior_layer": (_I, [_P, _P, _I, _P, _P, _I, _I, _I, _P, _P, _P, _I, _P, _P, _P, _SZ]),
    "stts_op_flow_stats_layer": (_I, [_P, _P, _I, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _SZ]),
}

_lib = None


def load() -> C.CDLL:
    """Load the shared library (no GPU needed for loading / symbol checks)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback."
        )
    # One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64 (same SONAME, libamdhip64.so.7, as
    # the system one this library is linked against).  If this library were loaded first the system copy would come in,
    # torch would then add its own, and whichever initialises second reports "no ROCm-capable device".  Importing torch
    # first makes the dynamic loader resolve our dependency to the copy torch already loaded.
    try:
        import torch  # noqa: F401
    except ImportError:  # pure C-ABI use without PyTorch: the system runtime is the only one
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in TEST_SIGNATURES.items():  # a product-only build (STTS_PRODUCT_ONLY=1) has none of these
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError("stylish_hip: " + (load().stts_last_error() or b"?").decode("utf-8", "replace"))
