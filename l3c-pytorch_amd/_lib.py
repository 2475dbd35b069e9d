"""ctypes binding of the C ABI in include/l3c_hip.h (libl3c_hip.so, built by csrc/build.py).

This is the reference-side binding a maintainer would add in place of `import torchac_backend_gpu`
(src/torchac/torchac.py:36-48): raw device pointers (`tensor.data_ptr()`), sizes, and the current HIP stream.
There is no CPU implementation behind it: a missing library or a CPU tensor raises.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# L3C_LIB: a development build of the same library (e.g. the -DL3C_WINO_TIMELINE one of csrc/build.py --timeline)
LIB_PATH = os.environ.get('L3C_LIB') or os.path.join(_HERE, 'csrc', 'libl3c_hip.so')

c_i64, c_int, c_vp, c_f32 = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_float


class L3CError(RuntimeError):
    pass


class ConvDesc(ctypes.Structure):
    """l3c_conv_desc (include/l3c_hip.h)."""
    _fields_ = [('inp', c_vp), ('in_cstride', c_int), ('in_coff', c_int),
                ('packed_w', c_vp), ('bias', c_vp),
                ('residual', c_vp), ('res_cstride', c_int), ('res_coff', c_int),
                ('out', c_vp), ('out_cstride', c_int), ('out_coff', c_int),
                ('B', c_int), ('Hin', c_int), ('Win', c_int), ('Cin', c_int), ('Cout', c_int),
                ('KS', c_int), ('stride', c_int), ('dilation', c_int), ('epilogue', c_int)]


class AcGroup(ctypes.Structure):
    """l3c_ac_group (include/l3c_hip.h)."""
    _fields_ = [('intervals', c_vp), ('out', c_vp), ('out_nbytes', c_vp),
                ('n_streams', c_i64), ('n_sym', c_i64), ('out_stride_bytes', c_i64)]


class ContainerScale(ctypes.Structure):
    """l3c_container_scale (include/l3c_hip.h)."""
    _fields_ = [('out', c_vp), ('nbytes', c_vp), ('stride', c_i64), ('C', c_int), ('H', c_int), ('W', c_int)]


class AcDecodePart(ctypes.Structure):
    """l3c_ac_decode_part (include/l3c_hip.h)."""
    _fields_ = [('cdf', c_vp), ('Lp', c_int), ('in_', c_vp), ('in_offsets', c_vp), ('in_nbytes', c_vp),
                ('n_streams', c_i64), ('n_sym', c_i64), ('not_monotone_flag', c_vp), ('state_in', c_vp),
                ('state_out', c_vp), ('final_chunk', c_int), ('sym_out', c_vp), ('sym_stride', c_i64), ('sym_offset', c_i64),
                ('window_stats_in', c_vp), ('window_stats_out', c_vp), ('P', c_vp), ('sym_all', c_vp), ('targets', c_vp),
                ('HW', c_i64), ('pix0', c_i64), ('C', c_int), ('K', c_int), ('c', c_int),
                ('r_npix', c_vp), ('r_table_off', c_vp), ('r_pixbase', c_vp), ('r_hw', c_vp), ('r_pix0', c_vp),
                ('r_C', c_int), ('r_c', c_int), ('r_table_bytes', c_i64)]


class TablePart(ctypes.Structure):
    """l3c_table_part (include/l3c_hip.h)."""
    _fields_ = [('c', c_int), ('pix0', c_i64), ('npix', c_i64), ('cdf', c_vp), ('not_monotone', c_vp), ('window_stats', c_vp)]


class RgbDecodeDesc(ctypes.Structure):
    """l3c_rgb_decode_desc (include/l3c_hip.h)."""
    _fields_ = [('P', c_vp), ('targets', c_vp), ('sym', c_vp), ('B', c_i64), ('HW', c_i64), ('K', c_int),
                ('in_', c_vp), ('in_offsets', c_vp), ('in_nbytes', c_vp), ('n_chunks', c_int),
                ('chunk_pix0_host', ctypes.POINTER(c_i64)), ('chunk_npix_host', ctypes.POINTER(c_i64)),
                ('lag', c_int), ('window_mode', c_int), ('workspace', c_vp), ('workspace_bytes', c_i64)]


class RaggedBatch(ctypes.Structure):
    """l3c_ragged_batch (include/l3c_hip.h)."""
    _fields_ = [('B', c_i64), ('max_hw', c_i64), ('pixbase', c_vp), ('hw', c_vp)]


class RaggedPart(ctypes.Structure):
    """l3c_ragged_part (include/l3c_hip.h)."""
    _fields_ = [('pix0', c_vp), ('npix', c_vp), ('table_off', c_vp)]


class RgbRaggedDesc(ctypes.Structure):
    """l3c_rgb_ragged_desc (include/l3c_hip.h)."""
    _fields_ = [('P', c_vp), ('targets', c_vp), ('sym', c_vp), ('B', c_i64), ('hw_host', ctypes.POINTER(c_i64)), ('K', c_int),
                ('in_', c_vp), ('in_offsets', c_vp), ('in_nbytes', c_vp), ('n_chunks', c_int),
                ('chunk_pix0_host', ctypes.POINTER(c_i64)), ('chunk_npix_host', ctypes.POINTER(c_i64)), ('tables_dev', c_vp),
                ('lag', c_int), ('window_mode', c_int), ('workspace', c_vp), ('workspace_bytes', c_i64)]


class BandedScale(ctypes.Structure):
    """l3c_banded_scale (include/l3c_hip.h)."""
    _fields_ = [('out_full', c_vp), ('nbytes_full', c_vp), ('stride_full', c_i64), ('out_last', c_vp), ('nbytes_last', c_vp),
                ('stride_last', c_i64), ('C', c_int), ('H', c_int), ('W', c_int), ('band_len', c_i64)]


class RgbBandedDesc(ctypes.Structure):
    """l3c_rgb_banded_desc (include/l3c_hip.h)."""
    _fields_ = [('P', c_vp), ('targets', c_vp), ('sym', c_vp), ('B', c_i64), ('HW', c_i64), ('K', c_int),
                ('in_', c_vp), ('in_offsets', c_vp), ('in_nbytes', c_vp), ('band_len', c_i64), ('n_chunks', c_int),
                ('lag', c_int), ('window_mode', c_int), ('workspace', c_vp), ('workspace_bytes', c_i64)]


class RgbEntriesDesc(ctypes.Structure):
    """l3c_rgb_entries_desc (include/l3c_hip.h)."""
    _fields_ = [('P', c_vp), ('targets', c_vp), ('sym', c_vp), ('S', c_i64), ('total_pix', c_i64), ('entries_dev', c_vp),
                ('entries_host', ctypes.POINTER(c_i64)), ('K', c_int), ('in_', c_vp), ('in_offsets', c_vp), ('in_nbytes', c_vp),
                ('n_chunks', c_int), ('lag', c_int), ('window_mode', c_int), ('workspace', c_vp), ('workspace_bytes', c_i64)]


NET_MAX_SCALES = 4    # include/l3c_hip.h: L3C_NET_MAX_SCALES


class NetConfig(ctypes.Structure):
    """l3c_net_config (include/l3c_hip.h)."""
    _fields_ = [('num_scales', c_int), ('Cf', c_int), ('C', c_int), ('L', c_int), ('K', c_int), ('enc_blocks', c_int),
                ('dec_blocks', c_int), ('rgb_baseline', c_int), ('dec_skip', c_int)]


class NetForwardDesc(ctypes.Structure):
    """l3c_net_forward_desc (include/l3c_hip.h)."""
    _fields_ = [('cfg_host', ctypes.POINTER(NetConfig)), ('packed', c_vp), ('packed_bytes', c_i64), ('img', c_vp), ('B', c_i64),
                ('H', c_int), ('W', c_int), ('sym', c_vp * (NET_MAX_SCALES + 1)), ('bn_q', c_vp * (NET_MAX_SCALES + 1)),
                ('P', c_vp * NET_MAX_SCALES), ('F_enc', c_vp * NET_MAX_SCALES), ('F_dec', c_vp * NET_MAX_SCALES),
                ('workspace', c_vp), ('workspace_bytes', c_i64)]


class NetGetPDesc(ctypes.Structure):
    """l3c_net_get_p_desc (include/l3c_hip.h)."""
    _fields_ = [('cfg_host', ctypes.POINTER(NetConfig)), ('packed', c_vp), ('packed_bytes', c_i64), ('net', c_int), ('bn_q', c_vp),
                ('B', c_i64), ('h', c_int), ('w', c_int), ('fuse', c_vp), ('P', c_vp), ('F', c_vp), ('workspace', c_vp),
                ('workspace_bytes', c_i64)]


class NetGetPRowsDesc(ctypes.Structure):
    """l3c_net_get_p_rows_desc (include/l3c_hip.h)."""
    _fields_ = [('cfg_host', ctypes.POINTER(NetConfig)), ('packed', c_vp), ('packed_bytes', c_i64), ('net', c_int), ('bn_q', c_vp),
                ('B', c_i64), ('h', c_int), ('w', c_int), ('fuse', c_vp), ('c0', c_int), ('c1', c_int), ('P', c_vp), ('workspace', c_vp),
                ('workspace_bytes', c_i64)]


class CodecModel(ctypes.Structure):
    """l3c_codec_model (include/l3c_hip.h)."""
    _fields_ = [('cfg_host', ctypes.POINTER(NetConfig)), ('packed', c_vp), ('packed_bytes', c_i64), ('targets_rgb', c_vp),
                ('targets_z', c_vp), ('uniform_row', c_vp), ('z_x_min', c_f32), ('z_bin_width', c_f32)]


class EncodeBatchDesc(ctypes.Structure):
    """l3c_encode_batch_desc (include/l3c_hip.h)."""
    _fields_ = [('model_host', ctypes.POINTER(CodecModel)), ('img', c_vp), ('B', c_i64), ('H', c_int), ('W', c_int), ('padding', c_vp),
                ('files', c_vp), ('file_stride', c_i64), ('file_bytes', c_vp), ('workspace', c_vp), ('workspace_bytes', c_i64)]


class DecodeBatchDesc(ctypes.Structure):
    """l3c_decode_batch_desc (include/l3c_hip.h)."""
    _fields_ = [('model_host', ctypes.POINTER(CodecModel)), ('files', c_vp), ('plan_host', c_vp), ('plan', c_vp), ('plan_bytes', c_i64),
                ('pixels', c_vp), ('sym', c_vp), ('workspace', c_vp), ('workspace_bytes', c_i64)]


class U8Image(ctypes.Structure):
    """l3c_u8_image (include/l3c_hip.h): one image inside a byte buffer and its place in the padded frame."""
    _fields_ = [('offset', c_i64), ('row_stride', c_i64), ('chan_stride', c_i64), ('pix_stride', ctypes.c_int32), ('h', ctypes.c_int32),
                ('w', ctypes.c_int32), ('top', ctypes.c_int32), ('left', ctypes.c_int32)]


class U8Span(ctypes.Structure):
    """l3c_u8_span (include/l3c_hip.h): bytes [offset, offset + bytes) of a buffer."""
    _fields_ = [('offset', c_i64), ('bytes', c_i64)]


class RebuildGroup(ctypes.Structure):
    """l3c_rebuild_group (include/l3c_hip.h): one group of l3c_band_rebuild."""
    _fields_ = [('first_src', c_i64), ('n_rows', ctypes.c_int32), ('n_members', ctypes.c_int32), ('t', ctypes.c_int32),
                ('reserved', ctypes.c_int32), ('out', U8Span * 4)]


class RepairGroup(ctypes.Structure):
    """l3c_repair_group (include/l3c_hip.h): one group of a repair round."""
    _fields_ = [('file', ctypes.c_int32), ('c', ctypes.c_int32), ('g', ctypes.c_int32), ('t', ctypes.c_int32), ('r0', ctypes.c_int32),
                ('bands', ctypes.c_int32 * 4)]


class DecodeRepairRoundDesc(ctypes.Structure):
    """l3c_decode_repair_round_desc (include/l3c_hip.h)."""
    _fields_ = [('model_host', ctypes.POINTER(CodecModel)), ('plan_host', c_vp), ('round_host', c_vp), ('round', c_vp), ('round_bytes', c_i64),
                ('rows', c_vp), ('rows_bytes', c_i64), ('workspace', c_vp), ('workspace_bytes', c_i64), ('sym', c_vp), ('pixels', c_vp),
                ('crc_out', c_vp), ('round_workspace', c_vp), ('round_workspace_bytes', c_i64)]


class EncodeImagesDesc(ctypes.Structure):
    """l3c_encode_images_desc (include/l3c_hip.h)."""
    _fields_ = [('model_host', ctypes.POINTER(CodecModel)), ('src', c_vp), ('src_bytes', c_i64), ('images_host', c_vp), ('images', c_vp),
                ('B', c_i64), ('Hp', c_int), ('Wp', c_int), ('bands', c_int), ('files', c_vp), ('file_stride', c_i64), ('file_bytes', c_vp),
                ('workspace', c_vp), ('workspace_bytes', c_i64)]


class DecodeImagesDesc(ctypes.Structure):
    """l3c_decode_images_desc (include/l3c_hip.h)."""
    _fields_ = [('model_host', ctypes.POINTER(CodecModel)), ('files', c_vp), ('plan_host', c_vp), ('plan', c_vp), ('plan_bytes', c_i64),
                ('dst', c_vp), ('dst_bytes', c_i64), ('images_host', c_vp), ('images', c_vp), ('sym', c_vp), ('workspace', c_vp),
                ('workspace_bytes', c_i64)]


class RegionBox(ctypes.Structure):
    """l3c_region_box (include/l3c_hip.h)."""
    _fields_ = [('y0', ctypes.c_int32), ('y1', ctypes.c_int32), ('x0', ctypes.c_int32), ('x1', ctypes.c_int32)]


class RegionInfo(ctypes.Structure):
    """l3c_region_info (include/l3c_hip.h)."""
    _fields_ = [('bands', ctypes.c_int32 * 2), ('n_bands', ctypes.c_int32), ('sym_rows', ctypes.c_int32 * 2), ('conv_rows', ctypes.c_int32 * 2),
                ('valid_rows', ctypes.c_int32 * 2), ('decoder_rows', ctypes.c_int32 * 2), ('frame_rows', ctypes.c_int32),
                ('n_chunks', ctypes.c_int32), ('lag', ctypes.c_int32), ('out_rows', ctypes.c_int32), ('out_cols', ctypes.c_int32),
                ('streams_used', c_i64), ('streams_total', c_i64), ('bytes_used', c_i64), ('bytes_total', c_i64)]


class DecodeRegionDesc(ctypes.Structure):
    """l3c_decode_region_desc (include/l3c_hip.h)."""
    _fields_ = [('model_host', ctypes.POINTER(CodecModel)), ('files', c_vp), ('plan_host', c_vp), ('plan', c_vp), ('plan_bytes', c_i64),
                ('region_host', c_vp), ('region', c_vp), ('region_bytes', c_i64), ('pixels', c_vp), ('workspace', c_vp),
                ('workspace_bytes', c_i64)]


class Seal(ctypes.Structure):
    """l3c_seal (include/l3c_hip.h)."""
    _fields_ = [('generation', ctypes.c_uint16), ('frame_crc', ctypes.c_uint32), ('model_id', ctypes.c_uint64)]


class SealBands(ctypes.Structure):
    """l3c_seal_bands (include/l3c_hip.h); crc points into the file."""
    _fields_ = [('n', ctypes.c_int32), ('band_len', ctypes.c_uint32), ('crc', ctypes.c_void_p)]


class SealParity(ctypes.Structure):
    """l3c_seal_parity (include/l3c_hip.h); plen and payloads point into the file."""
    _fields_ = [('G', ctypes.c_int32), ('m', ctypes.c_int32), ('plen', ctypes.c_void_p), ('payloads', ctypes.c_void_p), ('payload_bytes', c_i64)]


class SealParityRS(ctypes.Structure):
    """l3c_seal_parity_rs (include/l3c_hip.h); plen and payloads point into the file."""
    _fields_ = [('G', ctypes.c_int32), ('m', ctypes.c_int32), ('R', ctypes.c_int32), ('plen', ctypes.c_void_p), ('payloads', ctypes.c_void_p),
                ('payload_bytes', c_i64)]


class SealHead(ctypes.Structure):
    """l3c_seal_head (include/l3c_hip.h): where the head part of an 'L3CH' section lies in its file."""
    _fields_ = [('at', c_i64), ('bytes', c_i64), ('check_ok', ctypes.c_int32), ('n_records', ctypes.c_int32)]


class SealParityDesc(ctypes.Structure):
    """l3c_seal_parity_desc (include/l3c_hip.h): everything l3c_seal_append_parity reads, all but scales_host and the offsets on the device."""
    _fields_ = [('files', c_vp), ('file_stride', c_i64), ('file_bytes', c_vp), ('B', c_i64), ('scales_host', ctypes.POINTER(BandedScale)),
                ('n_scales', ctypes.c_int32), ('G', ctypes.c_int32), ('R', ctypes.c_int32), ('head', ctypes.c_int32), ('reserved', ctypes.c_int32),
                ('padding', c_vp), ('model_id', ctypes.c_uint64), ('frame_crc', c_vp), ('band_crc', c_vp), ('parity', c_vp),
                ('parity_stride', c_i64), ('parity_nbytes', c_vp), ('head_parity', c_vp), ('head_parity_offset_host', ctypes.POINTER(c_i64)),
                ('head_parity_stride', c_i64), ('head_parity_nbytes', c_vp), ('payload_crc', c_vp), ('workspace', c_vp), ('workspace_bytes', c_i64)]


class ParityOpts(ctypes.Structure):
    """l3c_parity_opts (include/l3c_hip.h)."""
    _fields_ = [('G', ctypes.c_int32), ('R', ctypes.c_int32), ('head', ctypes.c_int32), ('reserved', ctypes.c_int32), ('model_id', ctypes.c_uint64)]


SEAL_BYTES = 24      # include/l3c_hip.h: L3C_SEAL_BYTES
EPI_RELU, EPI_RESIDUAL, EPI_PIXEL_SHUFFLE = 1, 2, 4
ABI_VERSION = 4      # include/l3c_hip.h: L3C_ABI_VERSION (4: grouped tables, l3c_decode_rgb, l3c_container_read; no canvas batches)

# name -> (restype, argtypes); must list every symbol include/l3c_hip.h declares (tests/test_abi.py checks)
PROTOTYPES = {
    'l3c_abi_version': (c_int, []),
    'l3c_bitstream_generation': (c_int, []),
    'l3c_last_error': (ctypes.c_char_p, []),
    'l3c_device_info': (c_int, [ctypes.c_char_p, c_int, ctypes.POINTER(c_int), ctypes.c_char_p, c_int]),
    'l3c_stream_create_cu_range': (c_int, [c_int, c_int, ctypes.POINTER(c_vp)]),
    'l3c_stream_create_cu_mask': (c_int, [ctypes.POINTER(ctypes.c_uint32), c_int, ctypes.POINTER(c_vp)]),
    'l3c_stream_destroy': (c_int, [c_vp]),
    'l3c_interval_words': (c_i64, [c_i64, c_i64]),
    'l3c_ac_intervals_from_table': (c_int, [c_vp, c_i64, c_int, c_vp, c_i64, c_i64, c_vp, c_vp]),
    'l3c_ac_max_bytes': (c_i64, [c_i64]),
    'l3c_ac_encode_workspace_bytes': (c_i64, [c_i64]),
    'l3c_ac_encode': (c_int, [c_vp, c_i64, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp]),
    'l3c_ac_encode_groups_workspace_bytes': (c_i64, [c_int, c_i64]),
    'l3c_ac_encode_groups': (c_int, [ctypes.POINTER(AcGroup), c_int, c_vp, c_vp]),
    'l3c_container_write': (c_int, [ctypes.POINTER(ContainerScale), c_int, c_i64, c_vp, c_vp, c_vp, c_vp]),
    'l3c_container_read': (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, ctypes.c_uint32, c_vp, c_vp]),
    'l3c_ac_band_intervals': (c_int, [c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp]),
    'l3c_container_write_banded_workspace_bytes': (c_i64, [ctypes.POINTER(BandedScale), c_int, c_i64]),
    'l3c_container_write_banded': (c_int, [ctypes.POINTER(BandedScale), c_int, c_i64, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    'l3c_decode_rgb_banded_workspace_bytes': (c_i64, [c_i64, c_i64, c_i64, c_int, c_int]),
    'l3c_decode_rgb_banded': (c_int, [ctypes.POINTER(RgbBandedDesc), c_vp, c_vp]),
    'l3c_decode_rgb_entries_workspace_bytes': (c_i64, [c_i64, ctypes.POINTER(c_i64), c_int, c_int]),
    'l3c_decode_rgb_entries': (c_int, [ctypes.POINTER(RgbEntriesDesc), c_vp, c_vp]),
    'l3c_dmll_cdf_table_parts': (c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_int, c_int, c_int, c_int, ctypes.POINTER(TablePart), c_int, c_vp]),
    'l3c_decode_rgb_workspace_bytes': (c_i64, [c_i64, c_i64, c_int, c_int]),
    'l3c_decode_rgb_stats_offset': (c_i64, [c_i64, c_i64, c_int, c_int]),
    'l3c_decode_rgb': (c_int, [ctypes.POINTER(RgbDecodeDesc), c_vp, c_vp]),
    'l3c_decode_rgb_ragged_workspace_bytes': (c_i64, [c_i64, c_i64, c_int, c_int]),
    'l3c_decode_rgb_ragged': (c_int, [ctypes.POINTER(RgbRaggedDesc), c_vp, c_vp]),
    'l3c_dmll_cdf_table_ragged': (c_int, [c_vp, c_vp, c_vp, ctypes.POINTER(RaggedBatch), c_int, c_int, c_int, c_int, ctypes.POINTER(TablePart),
                                          ctypes.POINTER(RaggedPart), c_int, c_vp]),
    'l3c_ac_decode_state_bytes': (c_i64, []),
    'l3c_ac_decode_chunks': (c_int, [ctypes.POINTER(AcDecodePart), c_int, c_vp]),
    'l3c_ac_decode': (c_int, [c_vp, c_i64, c_int, c_vp, c_vp, c_vp, c_i64, c_i64, c_int, c_vp, c_vp]),
    'l3c_cdf_check_monotone': (c_int, [c_vp, c_i64, c_int, c_vp, c_vp]),
    'l3c_dmll_channel_params': (c_int, [c_vp, c_vp, c_i64, c_i64, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp]),
    'l3c_cdf_table_mixture': (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_int, c_int, c_vp, c_vp, c_vp]),
    'l3c_dmll_encode_intervals': (c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_int, c_int, c_int, c_int, c_vp, c_vp]),
    'l3c_dmll_cdf_table': (c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_int, c_int, c_int, c_int, c_i64, c_i64, c_int, c_vp, c_vp, c_vp, c_vp]),
    'l3c_dmll_sample': (c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_int, c_int, c_int, c_vp, c_vp]),
    'l3c_dmll_mean': (c_int, [c_vp, c_i64, c_i64, c_int, c_int, c_int, c_f32, c_f32, c_int, c_vp, c_vp]),
    'l3c_dmll_conceal': (c_int, [c_vp, c_i64, c_i64, c_int, c_f32, c_f32, c_int, c_vp, c_vp, c_i64, c_vp, c_vp]),
    'l3c_dmll_nll': (c_int, [c_vp, c_vp, c_i64, c_i64, c_int, c_int, c_int, c_f32, c_f32, c_int, c_vp, c_vp]),
    'l3c_conv_packed_words': (c_i64, [c_int, c_int, c_int]),
    'l3c_conv_pack_weights': (c_int, [c_vp, c_int, c_int, c_int, c_vp, c_vp]),
    'l3c_conv_mfma': (c_int, [ctypes.POINTER(ConvDesc), c_vp]),
    'l3c_conv_wino4_packed_words': (c_i64, [c_int, c_int]),
    'l3c_conv_wino4_pack_weights': (c_int, [c_vp, c_int, c_int, c_vp, c_vp]),
    'l3c_conv_wino4': (c_int, [ctypes.POINTER(ConvDesc), c_vp]),
    'l3c_conv_wino4_phase': (c_int, [ctypes.POINTER(ConvDesc), c_int, c_int, c_vp]),
    'l3c_conv_wino4_stride2': (c_int, [ctypes.POINTER(ConvDesc), c_vp]),
    'l3c_conv_wino4_set_tiles_per_block': (c_int, [c_int]),
    'l3c_conv_pw_packed_words': (c_i64, [c_int, c_int]),
    'l3c_conv_pw_pack_weights': (c_int, [c_vp, c_int, c_int, c_vp, c_vp]),
    'l3c_conv_pw': (c_int, [ctypes.POINTER(ConvDesc), c_vp]),
    'l3c_conv_direct': (c_int, [ctypes.POINTER(ConvDesc), c_vp]),
    'l3c_rgb_head': (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp]),
    'l3c_to_q_quantize': (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp]),
    'l3c_dec_head': (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_int, c_int, c_vp, c_vp]),
    'l3c_meanshift_planar': (c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_vp, c_vp]),
    'l3c_rgb_to_u8': (c_int, [c_vp, ctypes.POINTER(c_f32), c_i64, c_i64, c_vp, c_vp]),
    'l3c_resample_u8': (c_int, [c_vp, c_i64, c_int, c_int, c_int, c_int, c_vp, c_vp, c_int, c_vp, c_vp]),
    'l3c_u8_to_sym_bn': (c_int, [c_vp, ctypes.POINTER(c_f32), c_i64, c_i64, c_vp, c_vp, c_vp]),
    'l3c_sym_to_bn': (c_int, [c_vp, c_i64, c_f32, c_f32, c_vp, c_vp]),
    'l3c_net_param_count': (c_int, [ctypes.POINTER(NetConfig)]),
    'l3c_net_param': (c_int, [ctypes.POINTER(NetConfig), c_int, ctypes.c_char_p, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_i64)]),
    'l3c_net_packed_bytes': (c_i64, [ctypes.POINTER(NetConfig)]),
    'l3c_net_pack_workspace_bytes': (c_i64, [ctypes.POINTER(NetConfig)]),
    'l3c_net_pack': (c_int, [ctypes.POINTER(NetConfig), ctypes.POINTER(c_vp), c_vp, c_i64, c_vp, c_i64, c_vp]),
    'l3c_net_forward_workspace_bytes': (c_i64, [ctypes.POINTER(NetConfig), c_i64, c_int, c_int]),
    'l3c_net_forward': (c_int, [ctypes.POINTER(NetForwardDesc), c_vp]),
    'l3c_net_get_p_workspace_bytes': (c_i64, [ctypes.POINTER(NetConfig), c_i64, c_int, c_int]),
    'l3c_net_get_p': (c_int, [ctypes.POINTER(NetGetPDesc), c_vp]),
    'l3c_container_layout': (c_int, [ctypes.POINTER(ContainerScale), c_int, c_i64, c_i64, c_vp, c_vp, c_vp]),
    'l3c_sym_to_u8': (c_int, [c_vp, c_i64, c_vp, c_vp]),
    'l3c_encode_file_stride': (c_i64, [ctypes.POINTER(NetConfig), c_int, c_int]),
    'l3c_encode_batch_workspace_bytes': (c_i64, [ctypes.POINTER(NetConfig), c_i64, c_int, c_int]),
    'l3c_encode_batch': (c_int, [ctypes.POINTER(EncodeBatchDesc), c_vp]),
    'l3c_decode_plan_bytes': (c_i64, [ctypes.POINTER(NetConfig), c_i64]),
    'l3c_decode_plan': (c_int, [ctypes.POINTER(NetConfig), c_vp, ctypes.POINTER(c_i64), c_i64, c_vp, c_i64, ctypes.POINTER(c_int),
                                ctypes.POINTER(c_int), c_vp]),
    'l3c_decode_batch_workspace_bytes': (c_i64, [ctypes.POINTER(NetConfig), c_vp]),
    'l3c_decode_batch': (c_int, [ctypes.POINTER(DecodeBatchDesc), c_vp, c_vp]),
    'l3c_ac_decode_bands': (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_int, c_vp, c_vp]),
    'l3c_container_layout_banded': (c_int, [ctypes.POINTER(BandedScale), c_int, c_i64, c_i64, c_vp, c_vp, c_vp]),
    'l3c_encode_banded_file_stride': (c_i64, [ctypes.POINTER(NetConfig), c_int, c_int, c_int]),
    'l3c_encode_batch_banded_workspace_bytes': (c_i64, [ctypes.POINTER(NetConfig), c_i64, c_int, c_int, c_int]),
    'l3c_encode_batch_banded': (c_int, [ctypes.POINTER(EncodeBatchDesc), c_int, c_vp]),
    'l3c_decode_plan_banded_bytes': (c_i64, [ctypes.POINTER(NetConfig), c_vp, ctypes.POINTER(c_i64), c_i64]),
    'l3c_decode_plan_banded': (c_int, [ctypes.POINTER(NetConfig), c_vp, ctypes.POINTER(c_i64), c_i64, c_vp, c_i64, ctypes.POINTER(c_int),
                                       ctypes.POINTER(c_int), c_vp]),
    'l3c_decode_batch_banded_workspace_bytes': (c_i64, [ctypes.POINTER(NetConfig), c_vp]),
    'l3c_decode_batch_banded_p_offset': (c_i64, [ctypes.POINTER(NetConfig), c_vp]),
    'l3c_decode_batch_banded': (c_int, [ctypes.POINTER(DecodeBatchDesc), c_vp, c_vp]),
    'l3c_decode_batch_banded_streams_offset': (c_i64, [ctypes.POINTER(NetConfig), c_vp]),
    'l3c_decode_plan_banded_stream': (c_int, [c_vp, c_int, c_i64, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64), ctypes.POINTER(ctypes.c_uint32)]),
    'l3c_band_rebuild': (c_int, [c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp]),
    'l3c_repair_coefficients': (c_int, [c_vp, c_int, c_int, c_vp, c_int, c_vp, c_vp]),
    'l3c_repair_round_plan_bytes': (c_i64, [ctypes.POINTER(NetConfig), c_vp]),
    'l3c_repair_round_plan': (c_int, [ctypes.POINTER(NetConfig), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, ctypes.POINTER(c_i64)]),
    'l3c_repair_round_groups': (c_int, [c_vp, ctypes.POINTER(ctypes.POINTER(RepairGroup)), ctypes.POINTER(c_i64),
                                        ctypes.POINTER(ctypes.POINTER(ctypes.c_int32)), ctypes.POINTER(c_i64)]),
    'l3c_decode_repair_round_workspace_bytes': (c_i64, [ctypes.POINTER(NetConfig), c_vp, c_vp]),
    'l3c_decode_repair_round': (c_int, [ctypes.POINTER(DecodeRepairRoundDesc), c_vp, c_vp]),
    'l3c_image_padding': (c_int, [c_int, c_int, c_int, c_vp]),
    'l3c_image_table_check': (c_int, [c_vp, c_i64, c_int, c_int, c_i64]),
    'l3c_u8_gather': (c_int, [c_vp, c_i64, c_vp, c_vp, c_i64, c_int, c_int, c_vp, c_vp, c_vp]),
    'l3c_u8_scatter': (c_int, [c_vp, c_i64, c_int, c_int, c_vp, c_i64, c_vp, c_vp, c_vp]),
    'l3c_encode_images_workspace_bytes': (c_i64, [ctypes.POINTER(NetConfig), c_i64, c_int, c_int, c_int]),
    'l3c_encode_images': (c_int, [ctypes.POINTER(EncodeImagesDesc), c_vp]),
    'l3c_decode_images_workspace_bytes': (c_i64, [ctypes.POINTER(NetConfig), c_vp]),
    'l3c_decode_images': (c_int, [ctypes.POINTER(DecodeImagesDesc), c_vp, c_vp]),
    'l3c_net_halo_rows': (c_int, [c_int]),
    'l3c_net_apron_rows': (c_int, [c_int]),
    'l3c_net_get_p_rows_workspace_bytes': (c_i64, [ctypes.POINTER(NetConfig), c_i64, c_int, c_int, c_int, c_int]),
    'l3c_net_get_p_rows': (c_int, [ctypes.POINTER(NetGetPRowsDesc), c_vp]),
    'l3c_decode_region_plan_bytes': (c_i64, [ctypes.POINTER(NetConfig), c_vp]),
    'l3c_decode_region_plan': (c_int, [ctypes.POINTER(NetConfig), c_vp, c_i64, c_vp, ctypes.POINTER(RegionBox), c_vp, c_i64,
                                       ctypes.POINTER(RegionInfo)]),
    'l3c_decode_region_workspace_bytes': (c_i64, [ctypes.POINTER(NetConfig), c_vp, c_vp]),
    'l3c_decode_region': (c_int, [ctypes.POINTER(DecodeRegionDesc), c_vp, c_vp]),
    'l3c_seal_find': (c_int, [c_vp, c_i64, ctypes.POINTER(c_i64), ctypes.POINTER(Seal)]),
    'l3c_seal_write': (c_int, [ctypes.POINTER(Seal), c_vp, c_vp]),
    'l3c_u8_crc32_workspace_bytes': (c_i64, [c_i64, c_i64]),
    'l3c_u8_crc32': (c_int, [c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_i64, c_vp]),
    'l3c_u8_crc32_tile': (c_int, [ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    'l3c_u8_crc32_spans_workspace_bytes': (c_i64, [c_vp, c_i64]),
    'l3c_u8_crc32_spans': (c_int, [c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp]),
    'l3c_seal_append': (c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, ctypes.c_uint64, c_i64, c_vp]),
    'l3c_seal_bands_bytes': (c_i64, [c_int]),
    'l3c_seal_find_bands': (c_int, [c_vp, c_i64, ctypes.POINTER(c_i64), ctypes.POINTER(Seal), ctypes.POINTER(SealBands)]),
    'l3c_seal_write_bands': (c_int, [ctypes.POINTER(Seal), c_vp, c_vp, c_int, ctypes.c_uint32, c_vp]),
    'l3c_u8_crc32_bands_workspace_bytes': (c_i64, [c_i64, c_int, c_i64, c_i64]),
    'l3c_u8_crc32_bands': (c_int, [c_vp, c_i64, c_int, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp]),
    'l3c_seal_append_bands': (c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_int, ctypes.c_uint32, c_vp, ctypes.c_uint64, c_i64, c_vp]),
    'l3c_seal_parity_bytes': (c_i64, [c_int, c_int, c_i64]),
    'l3c_seal_find_parity': (c_int, [c_vp, c_i64, ctypes.POINTER(c_i64), ctypes.POINTER(Seal), ctypes.POINTER(SealBands), ctypes.POINTER(SealParity)]),
    'l3c_seal_write_parity': (c_int, [ctypes.POINTER(Seal), c_vp, c_vp, c_int, ctypes.c_uint32, c_int, c_vp, c_vp, c_vp]),
    'l3c_seal_parity_rs_bytes': (c_i64, [c_int, c_int, c_int, c_i64]),
    'l3c_seal_find_parity_rs': (c_int, [c_vp, c_i64, ctypes.POINTER(c_i64), ctypes.POINTER(Seal), ctypes.POINTER(SealBands), ctypes.POINTER(SealParityRS)]),
    'l3c_seal_write_parity_rs': (c_int, [ctypes.POINTER(Seal), c_vp, c_vp, c_int, ctypes.c_uint32, c_int, c_int, c_vp, c_vp, c_vp]),
    'l3c_band_parity_groups': (c_int, [c_int, c_int]),
    'l3c_band_parity': (c_int, [ctypes.POINTER(BandedScale), c_i64, c_int, c_vp, c_i64, c_vp, c_vp]),
    'l3c_u8_xor_spans': (c_int, [c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp]),
    'l3c_band_parity_rs': (c_int, [ctypes.POINTER(BandedScale), c_i64, c_int, c_int, c_vp, c_i64, c_vp, c_vp]),
    'l3c_u8_gf_spans': (c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp]),
    'l3c_seal_find_head': (c_int, [c_vp, c_i64, ctypes.POINTER(SealHead)]),
    'l3c_head_parity': (c_int, [ctypes.POINTER(BandedScale), c_int, c_i64, c_int, c_int, c_vp, c_vp, c_i64, c_vp, c_vp]),
    'l3c_band_payload_crc32': (c_int, [ctypes.POINTER(BandedScale), c_int, c_i64, c_vp, c_vp]),
    'l3c_seal_append_parity_workspace_bytes': (c_i64, [ctypes.POINTER(BandedScale), c_int, c_i64, c_int, c_int, c_int]),
    'l3c_seal_append_parity': (c_int, [ctypes.POINTER(SealParityDesc), c_vp]),
    'l3c_encode_banded_parity_file_stride': (c_i64, [ctypes.POINTER(NetConfig), c_int, c_int, c_int, ctypes.POINTER(ParityOpts)]),
    'l3c_encode_batch_banded_parity_workspace_bytes': (c_i64, [ctypes.POINTER(NetConfig), c_i64, c_int, c_int, c_int, ctypes.POINTER(ParityOpts)]),
    'l3c_encode_batch_banded_parity': (c_int, [ctypes.POINTER(EncodeBatchDesc), c_int, ctypes.POINTER(ParityOpts), c_vp]),
}

# include/l3c_xcheck.h: the TEST-ONLY cross-check library (round-1/2 Winograd F(2x2,3x3) kernel); see load_xcheck()
XCHECK_PROTOTYPES = {
    'l3c_conv_wino_packed_words': (c_i64, [c_int, c_int]),
    'l3c_conv_wino_pack_weights': (c_int, [c_vp, c_int, c_int, c_vp, c_vp]),
    'l3c_conv_wino': (c_int, [ctypes.POINTER(ConvDesc), c_vp]),
    'l3c_conv_wino_set_tiles_per_block': (c_int, [c_int]),
    'l3c_xcheck_sigmoid_exhaustive': (c_int, [c_vp, c_vp, c_vp]),
    'l3c_conv_wino4w_packed_words': (c_i64, [c_int, c_int]),
    'l3c_conv_wino4w_pack_weights': (c_int, [c_vp, c_int, c_int, c_vp, c_vp]),
    'l3c_conv_wino4w': (c_int, [ctypes.POINTER(ConvDesc), c_int, c_vp]),
}
# include/l3c_xcheck_small.h: the thin conv kernels before their streaming rewrite (csrc/xcheck_small.hip), same library
XCHECK_SMALL_PROTOTYPES = {
    'l3c_xcheck_rgb_head': (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp]),
    'l3c_xcheck_to_q_quantize': (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp]),
    'l3c_xcheck_dec_head': (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_int, c_int, c_vp, c_vp]),
    # the encoder's interval head before its vector fill and compile-time shapes (csrc/xcheck_iv.hip)
    'l3c_xcheck_dmll_encode_intervals': (c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_int, c_int, c_int, c_int, c_vp, c_vp]),
}
XCHECK_LIB_PATH = os.environ.get('L3C_XCHECK_LIB') or os.path.join(_HERE, 'csrc', 'libl3c_hip_xcheck.so')   # (L3C_XCHECK_LIB: a development variant)

_lib = None
_xcheck = None


def load():
    """The shared library, with prototypes installed.  Raises L3CError when it has not been built."""
    global _lib
    if _lib is None:
        _snapshot_queues()
        if not os.path.isfile(LIB_PATH):
            raise L3CError('libl3c_hip.so not found at {} -- build it with `python l3c-pytorch_amd/csrc/build.py` '
                           '(or __graft_entry__.build()); there is no CPU fallback.'.format(LIB_PATH))
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        if lib.l3c_abi_version() != ABI_VERSION:
            raise L3CError('ABI version mismatch: library {} != binding {}'.format(lib.l3c_abi_version(), ABI_VERSION))
        _lib = lib
    return _lib


def load_xcheck():
    """libl3c_hip_xcheck.so -- for tests and development probes ONLY: an independent second implementation of the 3x3 convolution
    to compare the product's kernels with.  Nothing under l3c-pytorch_amd/ calls this on the product path."""
    global _xcheck
    if _xcheck is None:
        if not os.path.isfile(XCHECK_LIB_PATH):
            raise L3CError('libl3c_hip_xcheck.so not found at {} -- build it with `python l3c-pytorch_amd/csrc/build.py`'.format(XCHECK_LIB_PATH))
        lib = ctypes.CDLL(XCHECK_LIB_PATH)
        lib.l3c_last_error.restype = ctypes.c_char_p
        for name, (res, args) in list(XCHECK_PROTOTYPES.items()) + list(XCHECK_SMALL_PROTOTYPES.items()):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _xcheck = lib
    return _xcheck


def call_xcheck(name, *args):
    rc = getattr(load_xcheck(), name)(*args)
    if rc != 0:
        raise L3CError('libl3c_hip_xcheck: {} (status {})'.format(load_xcheck().l3c_last_error().decode(), rc))


def check(rc):
    if rc != 0:
        raise L3CError('libl3c_hip: {} (status {})'.format(load().l3c_last_error().decode(), rc))


def call(name, *args):
    check(getattr(load(), name)(*args))


def _snapshot_queues():
    # the package's first HIP touch: remember what GPU_MAX_HW_QUEUES said when the runtime (may have) started -- helpers/runtime.py
    from .helpers import runtime
    runtime.snapshot_hw_queues()


def require_gpu():
    _snapshot_queues()
    if not torch.cuda.is_available():
        raise L3CError('no HIP device visible: the l3c-pytorch_amd compute path runs on the GPU only (no CPU fallback)')


def ptr(t, dtype=None):
    """Device pointer of a contiguous CUDA(HIP) tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise L3CError('expected a GPU tensor, got {} -- there is no CPU fallback'.format(t.device))
    if not t.is_contiguous():
        raise L3CError('expected a contiguous tensor')
    if dtype is not None and t.dtype != dtype:
        raise L3CError('expected dtype {}, got {}'.format(dtype, t.dtype))
    return t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def cu_range_stream(first_cu, n_cu):
    """torch stream object whose kernels are confined to CUs [first_cu, first_cu + n_cu)."""
    require_gpu()
    h = c_vp()
    call('l3c_stream_create_cu_range', first_cu, n_cu, ctypes.byref(h))
    return torch.cuda.ExternalStream(h.value)


def cu_mask_stream(cus):
    """torch stream object whose kernels are confined to the compute units listed in `cus` (hipExtStreamCreateWithCUMask)."""
    require_gpu()
    _, n_cu, _ = device_info()
    words = (ctypes.c_uint32 * ((n_cu + 31) // 32))()
    for cu in cus:
        if not 0 <= cu < n_cu:
            raise L3CError('compute unit {} outside the device ({} CUs)'.format(cu, n_cu))
        words[cu >> 5] |= 1 << (cu & 31)
    h = c_vp()
    call('l3c_stream_create_cu_mask', words, len(words), ctypes.byref(h))
    return torch.cuda.ExternalStream(h.value)


def device_info():
    name = ctypes.create_string_buffer(256)
    arch = ctypes.create_string_buffer(256)
    ncu = c_int(0)
    call('l3c_device_info', name, 256, ctypes.byref(ncu), arch, 256)
    return name.value.decode(), ncu.value, arch.value.decode()
