"""The C ABI of libx264hip.so as Python sees it, stated once: a ctypes record for every typedef struct of include/x264hip.h,
x264hip_lookahead.h and x264hip_stream.h that Python fills or reads by field, and the prototype of every function those headers declare.

    RECORDS      C typedef name -> record (tables.py adds the seven of include/x264hip_tables.h)
    PROTOTYPES   function name -> "return:parameters", applied to the library by lib.open_library()

Nothing here reads a header: both are literal, and tests/test_cpu_abi_and_shard.py holds them to include/*.h -- every record's size,
every field's offset and size, every function's return type, parameter count and parameter classes.  This module imports nothing from the
package; frame.py, slice.py, stream.py, lookahead.py, mux.py and lib.py import their records from here."""
import ctypes as C

import numpy as np

# The per-macroblock arrays an x264hip_mb_state begins with, in the header's order: (field, element type, shape per macroblock; None: mvr,
# [8][n_mb][2] per chain).  slice.DeviceState reads them back by these.
STATE_FIELDS = [("mb_type", np.int8, ()), ("partition", np.int8, ()), ("sub_partition", np.int8, (4,)), ("ref", np.int8, (4,)), ("i4mode", np.int8, (16,)),
                ("i16mode", np.int8, ()), ("chroma_mode", np.int8, ()), ("qp", np.int8, ()), ("t8", np.int8, ()),
                ("mv", np.int16, (16, 2)), ("mvr", np.int16, None), ("cbp", np.int16, ()), ("nnz", np.uint8, (27,)),
                ("luma", np.int16, (256,)), ("luma_dc", np.int16, (16,)), ("chroma_dc", np.int16, (8,)), ("chroma_ac", np.int16, (128,)),
                ("cost_intra", np.int32, ()), ("cost_inter", np.int32, ()), ("cost_intra_alt", np.int32, ())]


# ---- include/x264hip.h ---------------------------------------------------------------------------------------------------------------

class Cfg(C.Structure):
    _fields_ = [("device", C.c_int), ("arena_bytes", C.c_size_t)]


class Dims(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("mb_w", C.c_int), ("mb_h", C.c_int),
                ("stride_y", C.c_int), ("stride_c", C.c_int), ("lines_y", C.c_int), ("lines_c", C.c_int),
                ("batch", C.c_int)]


class Picture(C.Structure):
    _fields_ = [("plane", C.c_void_p * 3), ("filtered", C.c_void_p * 4), ("lowres", C.c_void_p * 4),
                ("integral", C.c_void_p), ("stride_lowres", C.c_int), ("width_lowres", C.c_int),
                ("lines_lowres", C.c_int)]


class Surface(C.Structure):
    """One device-resident source surface of x264hip_picture_import."""
    _fields_ = [("element", C.c_int), ("csp", C.c_int), ("plane", C.c_void_p * 3), ("pitch", C.c_int * 3)]


class CqmTables(C.Structure):
    _fields_ = [("quant4_mf", C.c_uint16 * (4 * 52 * 16)), ("quant4_bias", C.c_uint16 * (4 * 52 * 16)),
                ("quant8_mf", C.c_uint16 * (2 * 52 * 64)), ("quant8_bias", C.c_uint16 * (2 * 52 * 64)),
                ("dequant4_mf", C.c_int32 * (4 * 6 * 16)), ("dequant8_mf", C.c_int32 * (2 * 6 * 64)),
                ("unquant4_mf", C.c_int32 * (4 * 52 * 16)), ("unquant8_mf", C.c_int32 * (2 * 52 * 64))]


class MeParams(C.Structure):
    _fields_ = [("range", C.c_int), ("cost_mv", C.c_void_p), ("cost_mv_range", C.c_int),
                ("centers", C.c_void_p), ("mvp", C.c_void_p), ("sad_surface", C.c_void_p),
                ("mv_range", C.c_int)]


class Me16Params(C.Structure):
    _fields_ = [("me_method", C.c_int), ("me_range", C.c_int), ("subme", C.c_int), ("chroma_me", C.c_int),
                ("mv_range", C.c_int), ("cost_mv", C.c_void_p), ("cost_mv_range", C.c_int),
                ("mvp", C.c_void_p), ("mvc", C.c_void_p), ("n_mvc", C.c_void_p), ("ref_cost", C.c_int * 8)]


class MbState(C.Structure):
    _fields_ = [(name, C.c_void_p) for name, _, _ in STATE_FIELDS] + \
               [("progress", C.c_void_p), ("poc", C.c_int), ("n_ref0", C.c_int), ("inv_ref_poc", C.c_int * 8), ("mvd", C.c_void_p),
                ("mv1", C.c_void_p), ("ref1", C.c_void_p), ("mvr1", C.c_void_p), ("mvd1", C.c_void_p), ("skipbp", C.c_void_p),
                ("ref_poc", C.c_int * 8)]


class SliceRd(C.Structure):
    """The raster-order variant of the sweep (RD levels, trellis, adaptive quantisation, the entropy coder in the loop)."""
    _fields_ = [("trellis", C.c_int), ("psy_rd", C.c_int), ("write", C.c_int), ("cabac_init_idc", C.c_int), ("i_frame", C.c_int),
                ("qp_min", C.c_int), ("qp_max", C.c_int), ("f_qpm", C.c_float), ("aq_offset", C.c_void_p), ("cost_mv_all", C.c_void_p),
                ("unquant4_mf", C.c_void_p), ("unquant8_mf", C.c_void_p), ("payload", C.c_void_p), ("payload_cap", C.c_int),
                ("payload_len", C.c_void_p), ("mb_bits", C.c_void_p), ("stale", C.c_void_p), ("i_frame_stride", C.c_int), ("psy_trellis", C.c_int), ("psy_carry", C.c_void_p),
                ("mb_carry", C.c_void_p)]


class SliceParams(C.Structure):
    _fields_ = [("slice_type", C.c_int), ("qp", C.c_int), ("chroma_qp_offset", C.c_int),
                ("me_method", C.c_int), ("me_range", C.c_int), ("subme", C.c_int), ("chroma_me", C.c_int), ("mv_range", C.c_int),
                ("fast_pskip", C.c_int), ("dct_decimate", C.c_int), ("cabac", C.c_int), ("transform8x8", C.c_int),
                ("analyse_inter", C.c_int), ("analyse_intra", C.c_int),
                ("quant4_mf", C.c_void_p), ("quant4_bias", C.c_void_p), ("quant8_mf", C.c_void_p), ("quant8_bias", C.c_void_p),
                ("dequant4_mf", C.c_void_p), ("dequant8_mf", C.c_void_p),
                ("cost_mv", C.c_void_p), ("cost_mv_range", C.c_int), ("poc", C.c_int), ("ref_poc", C.c_int * 8),
                ("mixed_refs", C.c_int), ("profile", C.c_void_p), ("noise_reduction", C.c_int), ("nr", C.c_void_p), ("lossless", C.c_int),
                ("rd", C.c_void_p), ("lowres_mv", C.c_void_p), ("b", C.c_void_p)]


class SliceB(C.Structure):
    """List 1 of a B slice and what direct prediction reads."""
    _fields_ = [("fref1", C.c_void_p), ("l1_state", C.c_void_p), ("ref1_poc", C.c_int), ("weightb", C.c_int), ("lowres_mv1", C.c_void_p),
                ("direct_spatial", C.c_int), ("direct_score", C.c_void_p)]


class NrState(C.Structure):
    """h->nr_residual_sum / nr_count / nr_offset of every chain (device)."""
    _fields_ = [("sum", C.c_void_p), ("count", C.c_void_p), ("offset", C.c_void_p)]


class ResidualParams(C.Structure):
    _fields_ = [("qp", C.c_int), ("qp_chroma", C.c_int), ("transform8x8", C.c_int), ("b_interlaced", C.c_int),
                ("quant4_mf", C.c_void_p), ("quant4_bias", C.c_void_p),
                ("quant8_mf", C.c_void_p), ("quant8_bias", C.c_void_p),
                ("dequant4_mf", C.c_void_p), ("dequant8_mf", C.c_void_p),
                ("mv4x4_out", C.c_void_p), ("ref_out", C.c_void_p)]


class DeblockParams(C.Structure):
    _fields_ = [("mb_type", C.c_void_p), ("qp", C.c_void_p), ("nnz", C.c_void_p), ("transform8x8", C.c_void_p),
                ("mv", C.c_void_p), ("ref", C.c_void_p),
                ("alpha_c0_offset", C.c_int), ("beta_offset", C.c_int), ("chroma_qp_offset", C.c_int),
                ("state_layout", C.c_int), ("sub8x8", C.c_int)]


class LookaheadParams(C.Structure):
    _fields_ = [("mb_w", C.c_int), ("mb_h", C.c_int), ("bframes", C.c_int), ("b_adapt", C.c_int), ("bframe_bias", C.c_int),
                ("keyint_max", C.c_int), ("keyint_min", C.c_int), ("scenecut_threshold", C.c_int), ("pre_scenecut", C.c_int),
                ("rc_method", C.c_int), ("qp_constant", C.c_int), ("rf_constant", C.c_float), ("ip_factor", C.c_float),
                ("pb_factor", C.c_float), ("qcompress", C.c_float), ("qp_min", C.c_int), ("qp_max", C.c_int), ("qp_step", C.c_int)]


class Need(C.Structure):
    _fields_ = [("b", C.c_int), ("p0", C.c_int), ("p1", C.c_int), ("do_search", C.c_int * 2), ("speculative", C.c_int)]


class Frame(C.Structure):
    _fields_ = [("frame", C.c_int), ("type", C.c_int), ("poc", C.c_int), ("kept_as_ref", C.c_int), ("qp", C.c_int), ("f_qpm", C.c_float),
                ("ref0_frame", C.c_int), ("ref1_frame", C.c_int), ("lowres_l0", C.c_int), ("lowres_l1", C.c_int), ("i_satd", C.c_int),
                ("frame_num_reset", C.c_int)]


class LookSlot(C.Structure):
    _fields_ = [("pic", C.c_void_p), ("intra_cost", C.c_void_p), ("mv", C.c_void_p), ("mv_cost", C.c_void_p)]


class LookTask(C.Structure):
    _fields_ = [("chain", C.c_int), ("slot_b", C.c_int), ("slot_p0", C.c_int), ("slot_p1", C.c_int), ("d0", C.c_int), ("d1", C.c_int),
                ("do_search", C.c_int * 2)]


class LookParams(C.Structure):
    _fields_ = [("me_method", C.c_int), ("me_range", C.c_int), ("weighted_bipred", C.c_int), ("bframes", C.c_int), ("bframe_bias", C.c_int),
                ("subme_param", C.c_int), ("lossless", C.c_int), ("cost_mv", C.c_void_p), ("cost_mv_range", C.c_int)]


# ---- include/x264hip_lookahead.h -----------------------------------------------------------------------------------------------------

class ChainSweep(C.Structure):
    _fields_ = [("chain", C.c_int), ("fenc", C.c_void_p), ("refs", C.c_void_p), ("n_refs", C.c_int), ("recon", C.c_void_p),
                ("params", C.c_void_p), ("l0", C.c_void_p), ("out", C.c_void_p)]


class CavlcParams(C.Structure):
    _fields_ = [("slice_type", C.c_int), ("n_ref0", C.c_int), ("analyse_inter", C.c_int), ("transform8x8", C.c_int), ("cqm_custom", C.c_int),
                ("payload", C.c_void_p), ("payload_cap", C.c_int), ("payload_len", C.c_void_p), ("mb_bits", C.c_void_p), ("slice_qp", C.c_int)]


class CabacParams(C.Structure):
    """One frame's slices for x264hip_cabac_write_frame: the CABAC writer as a pass behind the sweep."""
    _fields_ = [("slice_type", C.c_int), ("n_ref0", C.c_int), ("analyse_inter", C.c_int), ("transform8x8", C.c_int), ("slice_qp", C.c_int),
                ("cabac_init_idc", C.c_int), ("i_frame", C.c_int), ("i_frame_stride", C.c_int),
                ("payload", C.c_void_p), ("payload_cap", C.c_int), ("payload_len", C.c_void_p), ("mb_bits", C.c_void_p)]


class ChainCavlc(C.Structure):
    """One chain's slice in a launch of x264hip_cavlc_write_chains."""
    _fields_ = [("chain", C.c_int), ("state", C.c_void_p), ("params", C.c_void_p)]


# ---- include/x264hip_stream.h --------------------------------------------------------------------------------------------------------

class EncoderParams(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("fps_num", C.c_int), ("fps_den", C.c_int), ("level_idc", C.c_int), ("threads", C.c_int),
                ("frame_reference", C.c_int), ("keyint_max", C.c_int), ("keyint_min", C.c_int), ("scenecut_threshold", C.c_int), ("pre_scenecut", C.c_int),
                ("bframe", C.c_int), ("bframe_adaptive", C.c_int), ("bframe_bias", C.c_int), ("bframe_pyramid", C.c_int),
                ("deblocking_filter", C.c_int), ("deblocking_filter_alphac0", C.c_int), ("deblocking_filter_beta", C.c_int),
                ("cabac", C.c_int), ("cabac_init_idc", C.c_int), ("interlaced", C.c_int), ("cqm_preset", C.c_int),
                ("intra", C.c_uint), ("inter", C.c_uint),
                ("transform_8x8", C.c_int), ("weighted_bipred", C.c_int), ("direct_mv_pred", C.c_int), ("chroma_qp_offset", C.c_int),
                ("me_method", C.c_int), ("me_range", C.c_int), ("mv_range", C.c_int), ("subpel_refine", C.c_int), ("chroma_me", C.c_int),
                ("mixed_references", C.c_int), ("trellis", C.c_int), ("fast_pskip", C.c_int), ("dct_decimate", C.c_int), ("noise_reduction", C.c_int),
                ("psy_rd", C.c_float), ("psy_trellis", C.c_float), ("luma_deadzone", C.c_int * 2),
                ("rc_method", C.c_int), ("qp_constant", C.c_int), ("qp_min", C.c_int), ("qp_max", C.c_int), ("qp_step", C.c_int),
                ("rf_constant", C.c_float), ("ip_factor", C.c_float), ("pb_factor", C.c_float), ("qcompress", C.c_float),
                ("aq_mode", C.c_int), ("aq_strength", C.c_float), ("scaling_list", C.c_void_p * 6),
                ("d_valid", C.c_int), ("d_lossless", C.c_int), ("d_profile_idc", C.c_int), ("d_num_ref_frames", C.c_int), ("d_num_reorder_frames", C.c_int),
                ("d_log2_max_frame_num", C.c_int), ("d_log2_max_poc_lsb", C.c_int), ("d_mb_width", C.c_int), ("d_mb_height", C.c_int),
                ("d_pic_init_qp", C.c_int), ("d_log2_max_mv_length", C.c_int), ("d_psy_rd_fix8", C.c_int)]


class SliceHeader(C.Structure):
    _fields_ = [("nal_type", C.c_int), ("nal_ref_idc", C.c_int), ("slice_type", C.c_int), ("frame_num", C.c_int), ("idr_pic_id", C.c_int),
                ("poc", C.c_int), ("qp", C.c_int), ("n_ref0", C.c_int), ("n_ref1", C.c_int), ("direct_spatial", C.c_int), ("ref_frame_num", C.c_int * 16)]


class FrameReport(C.Structure):
    """What the quality pass leaves per coded frame: h->stat.frame's measurements and counters."""
    _fields_ = [("ssd", C.c_int64 * 3), ("ssim", C.c_double), ("qp_sum", C.c_int32), ("mb_count", C.c_int32 * 19), ("mb_partition", C.c_int32 * 17),
                ("mb_count_8x8dct", C.c_int32 * 2), ("mb_count_ref", (C.c_int32 * 32) * 2), ("reserved", C.c_int32)]


class ChainReport(C.Structure):
    """One chain's frame in a launch of x264hip_frame_report_chains."""
    _fields_ = [("chain", C.c_int), ("fenc", C.c_void_p), ("fenc_element", C.c_int), ("recon", C.c_void_p), ("recon_element", C.c_int),
                ("state", C.c_void_p), ("slice_type", C.c_int), ("psnr", C.c_int), ("ssim", C.c_int), ("count_refs", C.c_int)]


class StatFrame(C.Structure):
    _fields_ = [("slice_type", C.c_int), ("frame_size", C.c_int), ("nal_ref_idc", C.c_int), ("poc", C.c_int), ("frames_since_ref", C.c_int),
                ("direct_spatial", C.c_int)]


# C typedef name -> record; tables.py adds the seven of include/x264hip_tables.h
RECORDS = {"x264hip_cfg": Cfg, "x264hip_frame_dims": Dims, "x264hip_picture": Picture, "x264hip_surface": Surface, "x264hip_cqm_tables": CqmTables,
           "x264hip_me_params": MeParams, "x264hip_me16_params": Me16Params, "x264hip_mb_state": MbState, "x264hip_slice_rd": SliceRd,
           "x264hip_slice_params": SliceParams, "x264hip_slice_b": SliceB, "x264hip_nr_state": NrState, "x264hip_residual_params": ResidualParams,
           "x264hip_deblock_params": DeblockParams, "x264hip_lookahead_params": LookaheadParams, "x264hip_look_need": Need,
           "x264hip_look_frame": Frame, "x264hip_look_slot": LookSlot, "x264hip_look_task": LookTask, "x264hip_look_params": LookParams,
           "x264hip_chain_sweep": ChainSweep, "x264hip_cavlc_params": CavlcParams, "x264hip_cabac_params": CabacParams,
           "x264hip_chain_cavlc": ChainCavlc,
           "x264hip_encoder_params": EncoderParams, "x264hip_slice_header": SliceHeader, "x264hip_frame_report": FrameReport,
           "x264hip_chain_report": ChainReport, "x264hip_stat_frame": StatFrame}


# Every function the three headers declare, as "return:parameters" in the classes the declarations use --
#   p  pointer of any kind (records, arrays, handles, streams, events: all c_void_p, so byref(), ctypes arrays, buffers, c_void_p, None and
#      bare integer addresses at full width all pass)      i  int      z  size_t      f  float      v  void      s  const char *
CLASSES = {"p": C.c_void_p, "i": C.c_int, "z": C.c_size_t, "f": C.c_float, "v": None, "s": C.c_char_p}
PROTOTYPES = {
    # include/x264hip.h
    "x264hip_init": "i:p",
    "x264hip_shutdown": "v:",
    "x264hip_last_error": "s:",
    "x264hip_device_count": "i:",
    "x264hip_malloc": "p:z",
    "x264hip_free": "v:p",
    "x264hip_memcpy_h2d": "i:ppz",
    "x264hip_memcpy_d2h": "i:ppz",
    "x264hip_device_synchronize": "i:",
    "x264hip_host_alloc": "p:z",
    "x264hip_host_free": "v:p",
    "x264hip_memcpy_d2h_async": "i:ppzp",
    "x264hip_memcpy_h2d_async": "i:ppzp",
    "x264hip_mem_info": "i:pp",
    "x264hip_device_cus": "i:",
    "x264hip_stream_create": "p:",
    "x264hip_stream_destroy": "v:p",
    "x264hip_stream_synchronize": "i:p",
    "x264hip_event_create": "p:",
    "x264hip_event_destroy": "v:p",
    "x264hip_event_record": "i:pp",
    "x264hip_event_elapsed_ms": "f:pp",
    "x264hip_stream_wait_event": "i:pp",
    "x264_pixel_init_hip": "i:p",
    "x264_dct_init_hip": "i:p",
    "x264_zigzag_init_hip": "i:pi",
    "x264_quant_init_hip": "i:p",
    "x264_mc_init_hip": "i:p",
    "x264_predict_16x16_init_hip": "i:p",
    "x264_predict_8x8c_init_hip": "i:p",
    "x264_predict_4x4_init_hip": "i:p",
    "x264_predict_8x8_init_hip": "i:pp",
    "x264_deblock_init_hip": "i:p",
    "x264hip_frame_ctx_new": "p:pp",
    "x264hip_frame_ctx_delete": "v:p",
    "x264hip_frame_ctx_stream": "p:p",
    "x264hip_picture_alloc": "i:pp",
    "x264hip_picture_alloc_source": "i:pp",
    "x264hip_picture_copy_element": "i:ppipi",
    "x264hip_picture_free": "v:pp",
    "x264hip_sync": "i:p",
    "x264hip_frame_ctx_select": "i:pi",
    "x264hip_picture_upload": "i:pppipipi",
    "x264hip_picture_upload_async": "i:pppipipip",
    "x264hip_picture_import": "i:pppipp",
    "x264hip_surface_bytes": "z:",
    "x264hip_picture_synth": "i:ppii",
    "x264hip_picture_download": "i:ppipii",
    "x264hip_expand_border": "i:ppi",
    "x264hip_hpel_filter_frame": "i:pp",
    "x264hip_lowres_init_frame": "i:pp",
    "x264hip_lookahead_intra_frame": "i:ppp",
    "x264hip_lookahead_intra_frame_sad": "i:ppp",
    "x264hip_cost_mv_table": "v:iip",
    "x264hip_cqm_init": "i:ppip",
    "x264hip_unquant_table": "v:piip",
    "x264hip_nal_encode": "i:piiipi",
    "x264hip_aq_var_frame": "i:ppp",
    "x264hip_adaptive_quant_frame": "i:ppfpp",
    "x264hip_ssd_frame": "i:pppp",
    "x264hip_ssd_frame_async": "i:pppp",
    "x264hip_me_fullpel_frame": "i:pppppp",
    "x264hip_me_subpel_frame": "i:ppppppp",
    "x264hip_me_search16_frame": "i:pppipppp",
    "x264hip_nr_state_alloc": "i:pp",
    "x264hip_nr_state_free": "v:pp",
    "x264hip_noise_reduction_update": "i:ppi",
    "x264hip_noise_reduction_update_chains": "i:ppipi",
    "x264hip_mb_state_alloc": "i:pp",
    "x264hip_mb_state_alloc_ex": "i:ppi",
    "x264hip_mb_state_free": "v:pp",
    "x264hip_slice_sweep_frame": "i:pppipppp",
    "x264hip_slice_sweep_status": "i:pp",
    "x264hip_inter_residual_frame": "i:ppppppppppp",
    "x264hip_inter_residual_frame_mp": "i:pppippppppppp",
    "x264hip_probe_skip_frame": "i:ppppipp",
    "x264hip_deblock_frame": "i:ppp",
    "x264hip_lookahead_new": "p:p",
    "x264hip_lookahead_delete": "v:p",
    "x264hip_lookahead_put": "i:p",
    "x264hip_lookahead_get": "i:pippip",
    "x264hip_lookahead_set_cost": "v:piiiiiii",
    "x264hip_lookahead_end": "v:p",
    "x264hip_lookahead_scenecut": "i:p",
    "x264hip_lookahead_state_bytes": "z:",
    "x264hip_lookahead_save": "i:pp",
    "x264hip_lookahead_restore": "v:pp",
    "x264hip_lookahead_oldest_live": "i:p",
    "x264hip_lookahead_cost_frames": "i:ppipipppp",
    "x264hip_lookahead_task_bytes": "z:",
    # include/x264hip_lookahead.h
    "x264hip_picture_alloc_lookahead": "i:pp",
    "x264hip_slice_sweep_chains": "i:ppipp",
    "x264hip_chain_sweep_bytes": "z:",
    "x264hip_mb_state_clear_progress": "i:pp",
    "x264hip_slice_sweep_chains_events": "i:ppipppp",
    "x264hip_event_query": "i:p",
    "x264hip_stream_create_high_priority": "p:",
    "x264hip_stream_create_cu_range": "p:ii",
    "x264hip_frame_ctx_set_b_stream": "i:pp",
    "x264hip_frame_ctx_elements": "i:ppi",
    "x264hip_cavlc_write_frame": "i:ppp",
    "x264hip_cabac_write_frame": "i:ppp",
    "x264hip_cavlc_write_chains": "i:ppipp",
    "x264hip_chain_cavlc_bytes": "z:",
    "x264hip_cavlc_write_frame_mp": "i:pppp",
    "x264hip_cavlc_write_chains_mp": "i:ppippp",
    "x264hip_cavlc_mp_scratch_bytes": "z:pi",
    # include/x264hip_stream.h
    "x264hip_encoder_params_default": "v:p",
    "x264hip_validate_parameters": "i:p",
    "x264hip_param2string": "i:ppi",
    "x264hip_sps_write": "i:ppi",
    "x264hip_pps_write": "i:ppi",
    "x264hip_sei_version_write": "i:ppi",
    "x264hip_slice_nal": "i:pppipi",
    "x264hip_frame_stats": "i:ppp",
    "x264hip_scenecut_post": "i:piiiii",
    "x264hip_slice_nal_sized": "i:pppipip",
    "x264hip_frame_report_chains": "i:ppipppp",
    "x264hip_chain_report_bytes": "z:",
    "x264hip_frame_report_scratch_bytes": "z:p",
    "x264hip_frame_report_frame": "i:ppppiipppp",
    "x264hip_frame_report_frame_staging_bytes": "z:",
    "x264hip_stat_new": "p:pii",
    "x264hip_stat_delete": "v:p",
    "x264hip_stat_frame_end": "i:ppppi",
    "x264hip_stat_summary": "i:ppi",
    "x264hip_stat_frames": "i:p",
}
