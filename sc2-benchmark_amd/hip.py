"""ctypes binding of libsc2amd.so (the C-ABI declared in include/sc2_bottleneck.h).

PyTorch is plumbing here: it owns device memory and streams; every compute call below goes through
the C-ABI with raw pointers and the current HIP stream.  There is NO fallback: if the shared library
is missing, or a tensor is not on a HIP device, the call raises.
"""
import collections
import ctypes
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('SC2_LIB') or os.path.join(_HERE, 'libsc2amd.so')   # SC2_LIB: A/B builds (tools/)
_lib = None

AOP_NONE, AOP_ABS, AOP_SQUARE = 0, 1, 2
EPI_NONE, EPI_GDN, EPI_IGDN, EPI_BIAS, EPI_BIAS_RELU, EPI_BIAS_ADD_RELU, EPI_FUSED_GDN, EPI_FUSED_IGDN, \
    EPI_BIAS_LEAKY_RELU, EPI_GDN2, EPI_IGDN2 = range(11)
FUSABLE_GDN_CHANNELS = (32, 48, 64, 96)   # conv + GDN1 in one launch: one tile must hold every output channel
OUT_BF16_NHWC, OUT_F32_NCHW, OUT_F32_NHWC, OUT_I32_NCHW_SYM = 0, 1, 2, 3
EB_NOISE, EB_DEQUANTIZE = 0, 1
EB_PARAM_STRIDE = 64

# symbols the header declares; tests check each is exported
ABI_SYMBOLS = [
    'sc2_abi_version', 'sc2_last_error', 'sc2_device_count', 'sc2_policy_default', 'sc2_policy_set', 'sc2_policy_get',
    'sc2_nchw_f32_to_nhwc_bf16', 'sc2_nhwc_bf16_to_nchw_f32', 'sc2_avgpool_nhwc', 'sc2_maxpool_nhwc', 'sc2_bn_ws_floats', 'sc2_bn_train_fwd', 'sc2_bn_train_bwd', 'sc2_fc_fwd',
    'sc2_conv_weight_rows', 'sc2_conv_weight_pitch', 'sc2_conv_fused_gdn_supported', 'sc2_conv_patch_supported',
    'sc2_conv2d_fwd', 'sc2_gdn1_bwd_gemm', 'sc2_colsum_bf16', 'sc2_nchw_f32_to_nhwc_f32', 'sc2_conv_f32_chunk_channels', 'sc2_conv2d_f32_fwd',
    'sc2_conv_split_chunk_channels', 'sc2_conv2d_split_fwd',
    'sc2_conv2x2_gdn512_supported', 'sc2_conv2x2_gdn512_fwd', 'sc2_conv1x1_stream_supported', 'sc2_conv1x1_stream_mask_supported', 'sc2_conv1x1_stream_fwd', 'sc2_conv1x1_pair_supported', 'sc2_conv1x1_pair_fwd',
    'sc2_conv0_gdn96_supported', 'sc2_conv0_gdn96_fwd', 'sc2_conv0_gdn96_nchw_fwd', 'sc2_conv2_gdn48_supported', 'sc2_conv2_gdn48_fwd', 'sc2_conv2x2_c48_supported', 'sc2_conv2x2_c48_fwd', 'sc2_conv1x1_kres_supported', 'sc2_conv1x1_kres_fwd', 'sc2_conv1x1_win_supported', 'sc2_conv1x1_win_fwd', 'sc2_conv1x1_w8_supported', 'sc2_conv1x1_w8_fwd', 'sc2_conv3x3_win_supported', 'sc2_conv3x3_win_fwd', 'sc2_conv3x3s2_win_supported', 'sc2_conv3x3s2_win_fwd', 'sc2_conv2x2_win_supported', 'sc2_conv2x2_win_fwd', 'sc2_conv2x2_win_tail_supported', 'sc2_conv2x2_win_tail_fwd', 'sc2_conv2d_wgrad', 'sc2_gdn_bwd_pre', 'sc2_gdn_bwd_post', 'sc2_gdn1_rows_supported', 'sc2_gdn1_rows_fwd', 'sc2_gdn1_rows_bwd',
    'sc2_eb_forward', 'sc2_eb_backward', 'sc2_eb_bits_partial_len', 'sc2_eb_backward_planes_per_wg', 'sc2_eb_symbols', 'sc2_eb_dequantize',
    'sc2_gc_forward', 'sc2_gc_backward', 'sc2_gc_symbols_indexes', 'sc2_gc_dequantize',
    'sc2_pmf_to_quantized_cdf',
    'sc2_rans_max_bytes', 'sc2_rans_workspace_bytes', 'sc2_rans_encode_batch', 'sc2_rans_decode_batch', 'sc2_rans_decode_dequantize_batch', 'sc2_rans_decode_dequantize_batch_ev', 'sc2_rans_decode_path',
    'sc2_mse_partial_len', 'sc2_mse_sum_bf16', 'sc2_mse_grad_bf16', 'sc2_relu_bwd_bf16', 'sc2_relu_bwd_mse_bf16',
    'sc2_gdn_bwd_pre_blocks', 'sc2_colsum_blocks', 'sc2_gdn_bwd_post_blocks', 'sc2_layout_blocks', 'sc2_gdn1_rows_units', 'sc2_gdn1_rows_workgroups',
    'sc2_ar_scan', 'sc2_ar_scan_f32', 'sc2_rans_decode_resume',
    'sc2_bq_partial_len', 'sc2_bq_quantize', 'sc2_bq_dequantize', 'sc2_bq_dequantize_nhwc', 'sc2_maxpool_affine_relu_nhwc', 'sc2_avgpool2d_nhwc',
    'sc2_nms_ws_bytes', 'sc2_nms', 'sc2_roi_align', 'sc2_roi_align_backward', 'sc2_box_match_ws_bytes', 'sc2_box_match', 'sc2_det_postprocess_ws_bytes', 'sc2_det_postprocess', 'sc2_rpn_proposals_ws_bytes', 'sc2_rpn_proposals', 'sc2_seg_predict', 'sc2_seg_ce_ws_bytes', 'sc2_seg_ce_forward', 'sc2_seg_ce_backward', 'sc2_seg_augment_workspace', 'sc2_seg_augment', 'sc2_cls_input_workspace', 'sc2_cls_input', 'sc2_coco_match_ws_bytes', 'sc2_coco_match', 'sc2_coco_accumulate',
    'sc2_jpeg_max_bytes', 'sc2_jpeg_tensor_codec', 'sc2_jpeg_image_max_bytes', 'sc2_jpeg_image_workspace_bytes', 'sc2_jpeg_image_codec',
    'sc2_rcnn_resize_u8', 'sc2_rcnn_normalize_pad', 'sc2_det_input',
    'sc2_rans_host_tables_create', 'sc2_rans_host_tables_destroy', 'sc2_rans_host_rcp_div', 'sc2_rans_code_host', 'sc2_clock_probe', 'sc2_rans_encode_host', 'sc2_rans_decode_host',
]


class ConvDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        'N', 'H', 'W', 'Cin', 'Cout', 'KH', 'KW', 'stride_h', 'stride_w', 'pad_h', 'pad_w', 'OH', 'OW',
        'a_op', 'epilogue', 'out_format', 'Kpad', 'Cout_pad', 'out_H', 'out_W', 'out_stride_h', 'out_stride_w',
        'out_off_h', 'out_off_w', 'k_order', 'dil_h', 'dil_w')]


class ArScanArgs(ctypes.Structure):
    """sc2_ar_scan_args of include/sc2_bottleneck.h."""
    _fields_ = ([(n, ctypes.c_int32) for n in ('B', 'H', 'W', 'M', 'C1p', 'C2p', 'n_table', 'n_cdfs', 'cdf_stride', 'pix0',
                                               'pix1', 'decode')] +
                [('scale_bound', ctypes.c_float), ('cdf_entries', ctypes.c_int32), ('stride', ctypes.c_int64)] +
                [(n, ctypes.c_void_p) for n in ('wc', 'bc', 'w1', 'p1', 'w2', 'b2', 'w3', 'b3', 'scale_table', 'y_hat_pad',
                                                'y_hat_nhwc', 'y', 'symbols', 'indexes', 'buf', 'io_offset', 'io_nbytes',
                                                'cdfs', 'cdf_sizes', 'offsets', 'st_x', 'st_pos', 'status',
                                                'gaussian_params')])


NMS_MAX_BOXES = 16384      # SC2_NMS_MAX_BOXES
ROI_MAX_LEVELS = 5         # SC2_ROI_MAX_LEVELS
MATCH_CHUNK = 2048         # SC2_MATCH_CHUNK: candidates per workgroup of sc2_box_match's first launch
MATCH_CAND_PER_WG, MATCH_GT_TILE = 1024, 64     # ... per workgroup of its second launch; gt boxes staged at a time
DETPOST_MAX_CLASSES, DETPOST_MAX_DET = 128, 1024      # SC2_DETPOST_*: C (background included) and detections per image
DETPOST_MAX_SEG, DETPOST_MAX_CAND = 2048, 20480       # survivors of one class of an image / of an image
DETPOST_OVER_CAND, DETPOST_OVER_SEG = 1, 2            # status bits
RPNPOST_MAX_LEVELS, RPNPOST_MAX_PRE_NMS, RPNPOST_MAX_POST_NMS = 8, 2048, 2048     # SC2_RPNPOST_*: L, K (pre-NMS top-n per level), P (post-NMS top-n)
RPNPOST_MAX_KEYS, RPNPOST_MAX_ANCHORS = 16384, 2 ** 29     # sum over the levels of min(K, n_l) / the anchors of an image stay below this
SEG_MAX_CLASSES = 64       # SC2_SEG_MAX_CLASSES
SEG_CE_MEAN, SEG_CE_SUM, SEG_CE_NONE = 0, 1, 2     # SC2_SEG_CE_*
COCO_THRS, COCO_RECS, COCO_AREAS, COCO_MAXDETS = 10, 101, 4, 3     # SC2_COCO_*
COCO_TILE_DETS, COCO_TILE_GTS, COCO_SCAN_CHUNK = 100, 64, 1024
JPEG_MAX_SIDE = 64         # SC2_JPEG_MAX_SIDE
JPEG_GREY, JPEG_RGB = 0, 1
JPEG_HEADER_BYTES = {0: 328, 1: 623}     # SC2_JPEG_HEADER_GREY / _RGB: a file is header + segment + 2
JPEG_NEGATIVE_MIN, JPEG_ZERO_MAX, JPEG_NOT_FINITE = 1, 2, 4     # SC2_JPEG_* status bits
JPEG_IMAGE_MAX_SIDE = 2048       # SC2_JPEG_IMAGE_MAX_SIDE
SEG_AUGMENT_DESC_INTS, SEG_AUGMENT_ENTRY_INTS = 16, 12      # SC2_SEG_AUGMENT_*
SEG_AUGMENT_MAX_SIDE, SEG_AUGMENT_MAX_BATCH = 16384, 65535
SEG_AUGMENT_RATIO, SEG_AUGMENT_BAD = 1, 2
CLS_INPUT_DESC_INTS, CLS_INPUT_MAX_BATCH = 16, 65535       # SC2_CLS_INPUT_*
CLS_INPUT_RATIO, CLS_INPUT_BAD, CLS_INPUT_TAP = 1, 2, 3
JPEG_IMAGE_CHUNK_BLOCKS = 128    # SC2_JPEG_IMAGE_CHUNK_BLOCKS
DET_INPUT_MAX_BATCH, DET_INPUT_ROW_INTS = 64, 6      # SC2_DET_INPUT_*
DET_INPUT_TILE_H, DET_INPUT_TILE_W = 16, 256


class RoiLevel(ctypes.Structure):
    """sc2_roi_level of include/sc2_bottleneck.h."""
    _fields_ = [('data', ctypes.c_void_p), ('H', ctypes.c_int32), ('W', ctypes.c_int32), ('spatial_scale', ctypes.c_float)]


class RoiLevels(ctypes.Structure):
    """sc2_roi_levels (passed by value)."""
    _fields_ = [('level', RoiLevel * ROI_MAX_LEVELS)]


class Sc2Error(RuntimeError):
    pass


# --------------------------------------------------------------------------------------------- #
# dispatch policy: no environment variable steers a kernel choice.  `Policy` mirrors `sc2_policy` of the
# C-ABI (the library's own choices), `HostPolicy` holds the choices made on this side of the boundary (which fused /
# persistent kernel a layer is sent to).  Defaults = the measured choices; `configure(name=value, ...)` changes either kind;
# tools/env_policy.py maps the SC2_* variables of the A/B scripts onto it -- the package itself never reads them.
# --------------------------------------------------------------------------------------------- #
POLICY_FIELDS = ('struct_bytes', 'conv_patch3', 'conv_s2', 'conv_persist', 'conv_half', 'conv_big4', 'conv_no_big', 'conv_force_big',
                 'conv_no_epx', 'conv_debug', 'conv_chunk', 'w2_run', 'win_half', 'win_dbg', 'win_stamps', 'p1_half',
                 'p1_nbuf', 'pair_alt', 'f32_persist0', 'dec_stagger', 'wgrad_wgs', 'rans_lds_pad_kb', 'rans_pad_waves', 'rans_ragged2',
                 'rans_ragged2_waves', 'rans_lut8', 'rans_dq_lds', 'wgrad_ct')


class Policy(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in POLICY_FIELDS] + [('reserved', ctypes.c_int32 * 6)]


class HostPolicy(object):
    """Kernel choices made in Python (per layer shape); every attribute is an A/B switch with its measured default."""
    conv_patch = True          # enc.conv2 + GDN48 on the LDS-patch tile kernel where the persistent kernel does not apply
    k_order_tap = False        # True: tap-major K everywhere (default: slab-major where several taps re-read pixels)
    b_tile_major = True        # weights packed [k-slab][row][32]
    conv0_fused = True         # conv0 + GDN96 as one persistent launch
    conv2_fused = True         # conv2 + GDN48 as one persistent launch
    conv_kres = 1              # weights-in-registers 1x1 kernel: 0 off, 1 the K = 1024 layers, 2 also K = 2048
    conv_win = True            # window-plane 3x3 kernel
    conv_win_s2 = True         # ... its stride-2 form
    conv2x2_win = True         # window-plane 2x2 decoder kernel
    w2_tail = True             # decoder's last conv takes layer2.0's conv1 + downsample along
    conv_stream = True         # persistent streaming 1x1 kernel
    conv1x1_pair = True        # conv3 + next block's conv1 in one launch
    conv_c48 = True            # streaming last encoder conv
    conv1x1_win = '1'          # window-plane 1x1 kernel: '0' none, '1' the layers it measured faster on, 'all'
    conv1x1_w8 = '1'           # eight-wave 256-channel 1x1 kernel: '0' none, '1' the layers it measured faster on (head._w8_policy), 'all'
    conv_dilation = True       # dilated layers through the descriptor's dilation (False: phase grids)
    fc_kernel = True           # dedicated classifier kernel
    dense_head = True          # DeepLab / FCN heads and the FPN on the library's kernels in bf16 eval
    rans_fused_dq = True       # decode + dequantise in one coder launch
    gdn_rows = True            # 96- / 256- / 512-channel GDN1 in training: forward and the whole backward on the resident-row kernel (gdn512_rows.hip)
    gdn_bwd_fused = True       # GDN1 backward: element-wise halves in the epilogues of its two GEMMs (sc2_gdn1_bwd_gemm)
    dgrad_win_halves = True    # data gradient of dec.conv2 as two 256-channel launches of the window-plane 2x2 kernel
    train_fused_conv2 = True   # training forward: encoder[2] + GDN1(48) as the fused inference launch that also emits the conv output
    train_fused_dec0 = True    # ... and decoder[0] + IGDN1(512) likewise (conv_gdn512.hip)
    train_fused_conv0 = True   # ... and encoder[0] + GDN1(96) (conv0_gdn96.hip, pixel-pair input)
    bn_train_hip = True        # BatchNorm2d (training mode) + ReLU + residual add of trainable Bottleneck blocks on sc2_bn_train_* (stage 2)
    conv_train_hip = True      # ... and their convolutions on autograd._ConvFn (forward, data and weight gradient on the library's kernels)
    pack_gather = True         # pack_conv_weight as one cast + one gather through a cached index map (False: the chain of layout ops)
    maxpool_hip = True         # nn.MaxPool2d behind a frozen stem (teacher, input-compression classifier) on sc2_maxpool_nhwc (False: torch's)
    relu_mask_fused = True     # the ReLU gradient behind a frozen block's conv2 / conv3 data gradient inside that launch's epilogue (window-plane kernels)
    mse_fused = True           # a feature-matching MSE term on a frozen stack's output: its gradient inside the stack's first ReLU-gradient pass
    teacher_stream = True      # distillation step: the frozen teacher's forward on a stream of its own beside the student's (+ 2 %)
    host_coder_max_streams = 64   # batches of up to this many streams go to the HOST range coder (bs-1 evaluation)
    head_ds_side_stream = False  # the head's downsample layers on a side stream beside conv1 -> conv2 of their block: measured SLOWER (head 2.60 -> 2.67 ms, bench - 1 %: profiles/r06e_ab_ds_side.txt)
    pipeline_host_steps = True   # StagePipeline(host_steps=None): the first batches of a run (up to 4, by the host's core count) are coded by the host thread pool while the device coder's first group is under way, their back stages gated behind the opening burst of front stages: + 1.5 - 2.5 % at K = 20 and K = 100 (profiles/r06o_host_steps_ab.txt); False: device coder only
    eval_graphs = True         # the updated eval forward of SplittableResNet at small batch replays HIP graphs of its device halves (graphs.py)
    eval_graph_max_batch = 1   # ... for batches up to this size (the reference evaluates at batch size 1)
    nms_hip = True             # detection.nms / batched_nms of device tensors on sc2_nms (False: the torch-op restatement, A/B)
    roi_align_hip = True       # detection.roi_align / multiscale_roi_align of device tensors on sc2_roi_align (False: torch ops, A/B)
    box_match_hip = True       # detection.match_boxes (the RPN's and the RoI heads' target assignment in training) of device tensors on sc2_box_match (False: the [G, A] `box_iou` matrix + `Matcher` on torch ops, A/B; tools/det_train_times.py, 6 images x 242 991 anchors x 20 gt boxes, 0.3 / 0.7 with low-quality matches: 0.17 against 2.41 ms, identical matches)
    roi_align_bwd_hip = True   # the backward of detection.multiscale_roi_align of f32 device maps on sc2_roi_align_backward (False: autograd through the torch-op restatement, forward included, A/B; tools/det_train_times.py, 3 072 RoIs over four maps of 6 images, C = 256, P = 7, S = 2: forward + backward 2.03 against 137.1 ms, the backward launch with its binning 1.64 ms)
    det_post_hip = True        # detection.RoIHeads.postprocess_detections of f32 device tensors on sc2_det_postprocess: three launches and one read-back per batch (False, or nms_hip off: softmax + decode, then the per-image loop of torch ops around batched_nms, A/B; a batch above the kernel's candidate caps takes that loop too; tools/det_post_times.py, 6 images x 1 000 proposals x 91 classes with 300 - 390 candidates per image above 0.05: 0.196 against 2.271 ms per batch, medians of 7 alternating rounds, the three launches alone 0.095 ms)
    rpn_post_hip = True        # detection.RegionProposalNetwork.forward of f32 device maps on sc2_rpn_proposals: three launches on the head's per-level maps as they stand and one read-back of the counts per batch (False, or nms_hip off: concat, decode of every anchor, topk per level, then filter_proposals' per-image loop of torch ops around batched_nms, A/B; other anchor generators and dimensions outside the kernel's caps take that path too; tools/rpn_post_times.py, 6 images x 242 991 anchors, all P proposals kept per image: 1.752 against 6.217 ms per batch at top-n 1 000, 2.884 against 11.254 ms at 2 000, medians of 7 alternating rounds, the three launches alone 1.264 / 2.349 ms; on by default: the whole existing GPU suite passes with it, the bit-identity of tests/test_gpu_detection.py's tail included)
    coco_eval_hip = True       # coco_eval.CocoBoxEvaluator.accumulate of device tensors on sc2_coco_match + sc2_coco_accumulate (False: the torch / numpy host path of the same module; tools/coco_eval_times.py)
    jpeg_codec_hip = True      # transforms.PILTensorModule(format='JPEG') of f32 device tensors up to 64 x 64 on sc2_jpeg_tensor_codec (False: PIL per channel group on the host, A/B; tools/jpeg_codec_times.py: 0.36 against 42.7 ms at [1,512,28,28])
    jpeg_image_hip = True      # transforms.PILImageModule(format='JPEG').forward_batch of equal-size RGB / grey PIL images up to 2048 x 2048 on sc2_jpeg_image_codec (False: PIL per image on the host, A/B; tools/jpeg_image_times.py, codec + ToTensor + Normalize to the classifier input: 0.39 against 0.50 ms at [1,3,224,224], 10.4 against 174 ms at [256,3,224,224])
    rcnn_input_hip = True      # detection.RCNNTransformWithCompression (eval, plain JPEG, f32 RGB device images): resize -> codec -> normalise + pad per image on sc2_rcnn_resize_u8 + sc2_jpeg_image_codec + sc2_rcnn_normalize_pad, one read-back per list (False: the reference's loop through Pillow on the host, A/B; tools/rcnn_input_times.py, 480 x 640 -> 800 x 1066 at quality 90: 2.79 against 25.7 ms at one image per call, 16.0 against 88.3 ms at six; the two new kernels alone 0.009 ms each, the codec 2.63 ms)
    seg_augment_hip = True     # transforms.DeferredSegBatch.materialize (the PASCAL CustomCompose chain, planned in the data-loader workers) on sc2_seg_augment: one copy up and two launches per batch (False: Pillow + torch on the host with the recorded draws, A/B; tools/seg_augment_times.py, 16 sources of 375 x 500 -> 513 x 513: 0.38 ms per batch with the copy up and the read-back, the launches alone 0.102 ms, against 86.0 ms through Pillow on one core)
    det_input_hip = True       # detection.GeneralizedRCNNTransform on a transforms.DeferredDetBatch (the COCO loader's ImageToTensor -> [flip] chain, planned in the data-loader workers) on sc2_det_input: one copy up of the source bytes and one launch per batch; coco_data.CustomCocoDetection plans its samples only while this is on (False: the float32 list of the host chain copied up, then normalise + F.interpolate + pad per image, A/B; tools/det_input_times.py, six 480 x 640 sources -> [6,3,800,1088]: 0.185 against 0.884 ms per batch with the copies up, the launch alone 0.042 ms)
    cls_input_hip = True       # transforms.DeferredClsBatch.materialize (the ImageNet train / eval chains of config.ImageFolder, planned in the data-loader workers) on sc2_cls_input: one copy up of the stored boxes and one launch per batch; config.ImageFolder plans its samples only while this is on (False: Pillow + ToTensor + Normalize per image in the worker and a float32 batch copied up, A/B; tools/cls_input_times.py, 256 decoded sources of 375 x 500 -> [256,3,224,224], one core: the worker's plan + pack 26.3 ms and materialize 3.6 ms with the copy up and the read-back against 271.5 ms per batch in the eval form, 21.6 + 2.9 against 182.9 ms in the train form; the launch alone 0.159 / 0.144 ms)
    seg_predict_hip = True     # dense.seg_labels (BaseSegmentationModel.predict, SegEvaluator.update_logits) of device tensors on sc2_seg_predict (False: interpolate + argmax + bincount, A/B)
    seg_loss_hip = True        # dense.seg_cross_entropy (DictLossWrapper over a deferred-resize segmentation student) of device tensors on sc2_seg_ce_forward + sc2_seg_ce_backward (False: F.interpolate + F.cross_entropy + autograd, A/B; tools/seg_loss_times.py, out + aux forward + backward at [8,21,65,65] -> 513 x 513: 1.27 against 2.70 ms with f32 logits, 1.27 against 1.72 ms with bf16, 20 against 707 MB of peak allocation)


host_policy = HostPolicy()


def get_policy():
    p = Policy()
    lib().sc2_policy_get(ctypes.byref(p))
    return p


def configure(**kw):
    """Sets dispatch-policy fields by name: fields of `sc2_policy` (the library) and attributes of `host_policy` (this side).
    -> the library policy in force.  Unknown names raise."""
    p = get_policy()
    touched = False
    for k, v in kw.items():
        if k in POLICY_FIELDS and k != 'struct_bytes':
            setattr(p, k, int(v))
            touched = True
        elif hasattr(HostPolicy, k):
            setattr(host_policy, k, v)
        else:
            raise Sc2Error('configure: unknown policy field {!r}'.format(k))
    if touched:
        _check(lib().sc2_policy_set(ctypes.byref(p)), 'policy_set')
    return p


def library_fingerprint():
    """{'lib_sha256': hash of the libsc2amd.so this process loads, 'csrc_sha256': hash of the kernel sources beside it (csrc/*.hip,
    *.h, *.cpp and include/sc2_bottleneck.h, names and contents in sorted order)}: what a committed measurement of the kernels
    (profiles/traffic.json) records, so that a reader -- bench.py -- can tell whether it still describes the library that runs.
    The source hash survives a rebuild (hipcc's output is not guaranteed to be byte-reproducible), the library hash a checkout
    without sources."""
    import hashlib
    out = {'lib_sha256': None, 'csrc_sha256': None}
    path = os.environ.get('SC2_LIB') or LIB_PATH
    if os.path.exists(path):
        h = hashlib.sha256()
        with open(path, 'rb') as f:
            for blk in iter(lambda: f.read(1 << 20), b''):
                h.update(blk)
        out['lib_sha256'] = h.hexdigest()
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, 'csrc')
    files = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(('.hip', '.h', '.cpp'))) if os.path.isdir(csrc) else []
    header = os.path.join(here, '..', 'include', 'sc2_bottleneck.h')
    if files and os.path.exists(header):
        h = hashlib.sha256()
        for f in files + [header]:
            h.update(os.path.basename(f).encode())
            h.update(open(f, 'rb').read())
        out['csrc_sha256'] = h.hexdigest()
    return out


def lib():
    """Loads libsc2amd.so; raises if it has not been built (python sc2-benchmark_amd/build.py)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise Sc2Error('libsc2amd.so not found at {}: the HIP extension is not built '
                       '(run `python -c "import __graft_entry__ as g; g.build()"`). '
                       'There is no CPU fallback.'.format(LIB_PATH))
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    L.sc2_abi_version.restype = i32
    L.sc2_last_error.restype = ctypes.c_char_p
    L.sc2_device_count.restype = i32
    L.sc2_policy_default.argtypes = [vp]
    L.sc2_policy_default.restype = None
    L.sc2_policy_set.argtypes = [vp]
    L.sc2_policy_get.argtypes = [vp]
    L.sc2_policy_get.restype = None
    L.sc2_nchw_f32_to_nhwc_bf16.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp]
    L.sc2_nhwc_bf16_to_nchw_f32.argtypes = [vp, vp, i32, i32, i32, i32, vp]
    L.sc2_avgpool_nhwc.argtypes = [vp, vp, vp, i32, i32, i32, vp]
    L.sc2_maxpool_nhwc.argtypes = [vp, vp] + [i32] * 10 + [vp]
    L.sc2_bn_ws_floats.argtypes = [ctypes.c_longlong, i32]
    L.sc2_bn_ws_floats.restype = ctypes.c_longlong
    L.sc2_bn_train_fwd.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.c_float, ctypes.c_float, i32, vp, vp, vp, vp, ctypes.c_longlong, i32, vp]
    L.sc2_bn_train_bwd.argtypes = [vp] * 11 + [ctypes.c_longlong, i32, vp]
    L.sc2_fc_fwd.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp]
    L.sc2_conv_weight_rows.argtypes = [i32]
    L.sc2_conv_weight_pitch.argtypes = [i32]
    L.sc2_conv_fused_gdn_supported.argtypes = [ctypes.POINTER(ConvDesc)]
    L.sc2_conv_patch_supported.argtypes = [ctypes.POINTER(ConvDesc)]
    L.sc2_conv2d_fwd.argtypes = [ctypes.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp]
    L.sc2_gdn1_bwd_gemm.argtypes = [ctypes.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp, vp]
    L.sc2_colsum_bf16.argtypes = [vp, ctypes.c_longlong, i32, vp, vp]
    L.sc2_nchw_f32_to_nhwc_f32.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp]
    L.sc2_conv_f32_chunk_channels.argtypes = [i32]
    L.sc2_conv2d_f32_fwd.argtypes = [ctypes.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp]
    L.sc2_conv_split_chunk_channels.argtypes = [i32]
    L.sc2_conv2d_split_fwd.argtypes = [ctypes.POINTER(ConvDesc), i32, vp, vp, vp, vp, vp, vp, vp]
    L.sc2_conv2x2_gdn512_supported.argtypes = [i32] * 6
    L.sc2_conv2x2_gdn512_fwd.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    L.sc2_conv0_gdn96_supported.argtypes = [i32, i32, i32]
    L.sc2_conv0_gdn96_fwd.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
    L.sc2_conv0_gdn96_nchw_fwd.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
    L.sc2_conv1x1_kres_supported.argtypes = [i32, i32, i32]
    L.sc2_conv1x1_kres_fwd.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
    L.sc2_conv3x3_win_supported.argtypes = [i32, i32, i32, i32]
    L.sc2_conv3x3_win_fwd.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
    L.sc2_conv3x3s2_win_supported.argtypes = [i32, i32, i32, i32]
    L.sc2_conv1x1_win_supported.argtypes = [i32, i32, i32]
    L.sc2_conv2x2_c48_supported.argtypes = [i32, i32, i32, i32]
    L.sc2_conv2x2_c48_fwd.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
    L.sc2_conv1x1_win_fwd.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
    L.sc2_conv1x1_w8_supported.argtypes = [i32, i32, i32]
    L.sc2_conv1x1_w8_fwd.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
    L.sc2_conv3x3s2_win_fwd.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
    L.sc2_conv2x2_win_supported.argtypes = [i32, i32, i32, i32, i32]
    L.sc2_conv2x2_win_fwd.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp]
    L.sc2_conv2x2_win_tail_supported.argtypes = [i32, i32, i32]
    L.sc2_conv2x2_win_tail_fwd.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
    L.sc2_conv2_gdn48_supported.argtypes = [i32, i32, i32]
    L.sc2_conv2_gdn48_fwd.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
    L.sc2_conv1x1_pair_supported.argtypes = [i32, i32, i32]
    L.sc2_conv1x1_pair_fwd.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_longlong, i32, i32, i32, vp]
    L.sc2_conv1x1_stream_supported.argtypes = [i32, i32, i32]
    L.sc2_conv1x1_stream_fwd.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
    L.sc2_conv1x1_stream_mask_supported.argtypes = [i32, i32, i32]
    L.sc2_conv2d_wgrad.argtypes = [ctypes.POINTER(ConvDesc), vp, vp, vp, vp]
    L.sc2_gdn1_rows_supported.argtypes = [i32]
    L.sc2_gdn1_rows_fwd.argtypes = [vp, vp, vp, vp, ctypes.c_longlong, i32, i32, vp]
    L.sc2_gdn1_rows_bwd.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_longlong, i32, i32, vp]
    L.sc2_gdn_bwd_pre.argtypes = [vp, vp, vp, ctypes.c_longlong, i32, i32, vp, vp, vp, vp]
    L.sc2_gdn_bwd_post.argtypes = [vp, vp, vp, ctypes.c_longlong, vp, vp]
    for name, args in (('sc2_gdn_bwd_pre_blocks', [ctypes.c_longlong, i32]), ('sc2_colsum_blocks', [ctypes.c_longlong, i32]),
                       ('sc2_gdn_bwd_post_blocks', [ctypes.c_longlong]), ('sc2_layout_blocks', [ctypes.c_longlong]),
                       ('sc2_gdn1_rows_units', [ctypes.c_longlong, i32]), ('sc2_gdn1_rows_workgroups', [ctypes.c_longlong, i32])):
        getattr(L, name).argtypes = args
        getattr(L, name).restype = ctypes.c_longlong
    L.sc2_eb_forward.argtypes = [vp, vp, vp, i32, i32, i32, i32, f32, vp, vp, vp, vp, i32, vp]
    L.sc2_eb_backward.argtypes = [vp, vp, vp, i32, i32, i32, i32, f32, vp, vp, vp, vp, i32, vp]
    L.sc2_eb_bits_partial_len.argtypes = [i32, i32, i32]
    L.sc2_eb_backward_planes_per_wg.argtypes = [i32, i32, i32]
    L.sc2_gc_forward.argtypes = [vp, vp, i64, vp, i64, vp, i64, i64, i32, f32, f32, vp, vp, vp]
    L.sc2_gc_backward.argtypes = [vp, vp, i64, vp, i64, vp, i64, i64, f32, f32, vp, vp, vp, vp, vp, vp]
    L.sc2_gc_symbols_indexes.argtypes = [vp, vp, i64, vp, i64, i64, i64, vp, i32, f32, vp, vp, vp]
    L.sc2_gc_dequantize.argtypes = [vp, vp, i64, i64, i32, i32, vp, vp, vp]
    L.sc2_eb_symbols.argtypes = [vp, vp, i32, i32, i32, vp, vp]
    L.sc2_eb_dequantize.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp]
    L.sc2_pmf_to_quantized_cdf.argtypes = [ctypes.POINTER(ctypes.c_float), i32, i32,
                                           ctypes.POINTER(ctypes.c_uint32)]
    L.sc2_rans_max_bytes.argtypes = [i64]
    L.sc2_rans_max_bytes.restype = i64
    L.sc2_rans_workspace_bytes.argtypes = [i32, i64, i32, i32]
    L.sc2_rans_workspace_bytes.restype = i64
    L.sc2_rans_encode_batch.argtypes = [vp, vp, i64, i32, i64, vp, i32, i32, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp]
    L.sc2_rans_decode_batch.argtypes = [vp, i64, vp, vp, vp, i64, i32, i64, vp, i32, i32, vp, vp, vp, vp, vp, i64,
                                        vp]
    L.sc2_rans_decode_dequantize_batch.argtypes = [vp, i64, vp, vp, i64, i32, i64, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, i64, vp]
    L.sc2_rans_decode_dequantize_batch_ev.argtypes = [vp, i64, vp, vp, i64, i32, i64, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp]
    L.sc2_rans_decode_path.argtypes = [i32, i64, i32, i64, i32, i32, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.sc2_mse_partial_len.argtypes = [ctypes.c_longlong]
    L.sc2_mse_sum_bf16.argtypes = [vp, vp, ctypes.c_longlong, vp, vp]
    L.sc2_mse_grad_bf16.argtypes = [vp, vp, ctypes.c_longlong, vp, vp, vp]
    L.sc2_relu_bwd_bf16.argtypes = [vp, vp, vp, ctypes.c_longlong, vp, vp]
    L.sc2_relu_bwd_mse_bf16.argtypes = [vp, vp, vp, vp, ctypes.c_longlong, i32, vp, vp]
    L.sc2_ar_scan.argtypes = [ctypes.POINTER(ArScanArgs), vp]
    L.sc2_ar_scan_f32.argtypes = [ctypes.POINTER(ArScanArgs), vp]
    L.sc2_rans_decode_resume.argtypes = [vp, i64, vp, vp, vp, i32, i64, vp, i32, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp]
    L.sc2_bq_partial_len.argtypes = [i64, i64]
    L.sc2_bq_partial_len.restype = i64
    L.sc2_bq_quantize.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, vp]
    L.sc2_bq_dequantize.argtypes = [vp, vp, vp, vp, i64, i64, vp]
    L.sc2_bq_dequantize_nhwc.argtypes = [vp, vp, vp, i32, vp, vp, i32, vp, i32, i32, i32, i32, i32, vp]
    L.sc2_maxpool_affine_relu_nhwc.argtypes = [vp, vp, vp, vp] + [i32] * 10 + [vp]
    L.sc2_avgpool2d_nhwc.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp]
    L.sc2_nms_ws_bytes.argtypes = [i32]
    L.sc2_nms_ws_bytes.restype = i64
    L.sc2_nms.argtypes = [vp, vp, i32, f32, vp, vp, vp, vp]
    L.sc2_roi_align.argtypes = [RoiLevels, i32, i32, i32, i32, vp, vp, i32, i32, i32, vp, vp]
    L.sc2_roi_align_backward.argtypes = [RoiLevels, i32, i32, i32, vp, vp, vp, vp, vp, i32, i32, i32, vp]
    L.sc2_box_match_ws_bytes.argtypes = [i32, i32]
    L.sc2_box_match_ws_bytes.restype = i64
    L.sc2_box_match.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, i32, vp, vp, vp, vp]
    L.sc2_det_postprocess_ws_bytes.argtypes = [i32, i32, i32, i32]
    L.sc2_det_postprocess_ws_bytes.restype = i64
    L.sc2_det_postprocess.argtypes = [vp] * 6 + [i32] * 3 + [f32] * 8 + [i32] + [vp] * 9
    L.sc2_rpn_proposals_ws_bytes.argtypes = [i32, i32, i32, i32]
    L.sc2_rpn_proposals_ws_bytes.restype = i64
    L.sc2_rpn_proposals.argtypes = [vp] * 5 + [i32] + [vp] * 2 + [i32] * 3 + [f32] * 8 + [vp] * 9
    L.sc2_seg_predict.argtypes = [vp, i32, i32, i32, i32, i32, i64, i64, i64, i64, i32, i32, i32, vp, vp, vp, vp]
    L.sc2_seg_ce_ws_bytes.argtypes = [i32, i32, i32]
    L.sc2_seg_ce_ws_bytes.restype = i64
    L.sc2_seg_ce_forward.argtypes = [vp, i32, i32, i32, i32, i32, i64, i64, i64, i64, i32, i32, i32, vp, i64, vp, vp, vp, vp, vp]
    L.sc2_seg_ce_backward.argtypes = [vp, i32, i32, i32, i32, i32, i64, i64, i64, i64, i32, i32, i32, vp, i64, vp, vp, vp, i32, vp, i64, i64, i64, i64, vp]
    L.sc2_coco_match_ws_bytes.argtypes = [i64]
    L.sc2_coco_match_ws_bytes.restype = i64
    L.sc2_coco_match.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    L.sc2_coco_accumulate.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]
    L.sc2_jpeg_max_bytes.argtypes = [i32, i32, i32]
    L.sc2_jpeg_max_bytes.restype = i64
    L.sc2_jpeg_tensor_codec.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, i64, vp]
    L.sc2_jpeg_image_max_bytes.argtypes = [i32, i32, i32]
    L.sc2_jpeg_image_max_bytes.restype = i64
    L.sc2_jpeg_image_workspace_bytes.argtypes = [i32, i32, i32, i32]
    L.sc2_jpeg_image_workspace_bytes.restype = i64
    L.sc2_jpeg_image_codec.argtypes = [vp, i64, i64, i64, i64, i32, i32, i32, i32, i32, vp, vp, vp, i64, vp, i64, vp]
    L.sc2_rcnn_resize_u8.argtypes = [vp, i64, i64, i64, i32, i32, i32, vp, i32, i32, vp, vp]
    L.sc2_rcnn_normalize_pad.argtypes = [vp, i32, i32, i32, vp, vp, vp, i32, i32, vp]
    L.sc2_det_input.argtypes = [vp, i64, vp, i32, vp, vp, vp, i32, i32, vp]
    L.sc2_seg_augment_workspace.argtypes = [i32, i32, i32]
    L.sc2_seg_augment_workspace.restype = i64
    L.sc2_seg_augment.argtypes = [vp, i64, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.sc2_cls_input_workspace.argtypes = [i32, i32, i32]
    L.sc2_cls_input_workspace.restype = i64
    L.sc2_cls_input.argtypes = [vp, i64, vp, i32, i32, i32, vp, vp, vp, vp, vp]
    L.sc2_rans_host_tables_create.argtypes = [vp, i32, i32, vp, vp, ctypes.POINTER(vp)]
    L.sc2_rans_host_tables_destroy.argtypes = [vp]
    L.sc2_rans_host_tables_destroy.restype = None
    L.sc2_rans_host_rcp_div.argtypes = [ctypes.c_uint64, ctypes.c_uint32]
    L.sc2_rans_host_rcp_div.restype = ctypes.c_uint64
    L.sc2_clock_probe.argtypes = [vp, i32, i32, ctypes.c_uint32, vp]
    L.sc2_rans_code_host.argtypes = [vp, vp, vp, i64, i32, i64, vp, i64, vp, vp, vp, vp, i32]
    L.sc2_rans_encode_host.argtypes = [vp, vp, vp, i64, i32, i64, vp, i64, vp, vp, vp, i32]
    L.sc2_rans_decode_host.argtypes = [vp, vp, i64, vp, vp, vp, i64, i32, i64, vp, vp, i32]
    for name in ABI_SYMBOLS:
        getattr(L, name)  # raises AttributeError if the library lacks a declared symbol
    _lib = L
    return L


def last_error():
    return lib().sc2_last_error().decode('utf-8', 'replace')


def _check(rc, what):
    if rc != 0:
        msg = last_error()
        if rc in (-1, -3, -4):
            raise ValueError('{}: {}'.format(what, msg))
        raise Sc2Error('{} failed (code {}): {}'.format(what, rc, msg))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class KernelTimer(object):
    """Optional HIP-event timing of individual launches, on the stream they are launched on.

    ``with hip.KernelTimer() as t: ...`` records an event pair around every launch made through this module
    whose tag passes ``select``; ``t.summary()`` (after a synchronize) returns {tag: (count, mean_ms)}.
    Used by bench.py to measure the dominant kernel live inside the timed region.
    """
    active = None

    def __init__(self, select=None):
        self.select = select
        self.records = []

    def __enter__(self):
        KernelTimer.active = self
        return self

    def __exit__(self, *exc):
        KernelTimer.active = None
        return False

    def summary(self):
        out = {}
        for rec in self.records:
            out.setdefault(rec[0], []).append(rec[1].elapsed_time(rec[2]))
        return {k: (len(v), sum(v) / len(v)) for k, v in out.items()}

    def total_ms(self, tag):
        """sum of the durations of every launch tagged `tag` (launches that cover different amounts of work, e.g. the coder's
        dequantise pass over 1, 2, 4 or 8 steps' streams, have no meaningful mean)."""
        return sum(rec[1].elapsed_time(rec[2]) for rec in self.records if rec[0] == tag)


class _timed(object):
    def __init__(self, tag):
        t = KernelTimer.active
        self.t = t if (t is not None and (t.select is None or t.select(tag))) else None
        self.tag = tag

    def __enter__(self):
        if self.t is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if self.t is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self.t.records.append((self.tag, self.e0, e1))
        return False


def _dev(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise Sc2Error('{} must be a tensor on a HIP device (got {}); there is no CPU fallback in this package'
                       .format(name, 'device=' + str(t.device) if isinstance(t, torch.Tensor) else type(t)))
    return t


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _pair2(v):
    """a stride / padding / dilation given as an int or as (h, w) -> (h, w)"""
    return (v, v) if isinstance(v, int) else v


def _fits32(*element_counts):
    """True if bf16 tensors of these element counts stay within the 32-bit byte offsets the buffer-addressed kernels use."""
    return max(element_counts) * 2 < 0x7FF00000


# --------------------------------------------------------------------------------------------- #
# layout
# --------------------------------------------------------------------------------------------- #
def nchw_f32_to_nhwc_bf16(x, cpad=None, tag=None):
    """x: f32 [N,C,H,W] contiguous -> bf16 tensor of shape [N,H,W,Cpad] (NHWC memory)."""
    _dev(x, 'x')
    assert x.dtype == torch.float32 and x.dim() == 4
    x = x.contiguous()
    N, C, H, W = x.shape
    cpad = C if cpad is None else cpad
    y = torch.empty((N, H, W, cpad), dtype=torch.bfloat16, device=x.device)
    with _timed(tag or 'layout.nchw_to_nhwc'):
        _check(lib().sc2_nchw_f32_to_nhwc_bf16(_ptr(x), _ptr(y), N, C, H, W, cpad, _stream()), 'nchw_f32_to_nhwc_bf16')
    return y


def nhwc_bf16_to_nchw_f32(x):
    """x: bf16 [N,H,W,C] -> f32 [N,C,H,W]."""
    _dev(x, 'x')
    assert x.dtype == torch.bfloat16 and x.dim() == 4 and x.is_contiguous()
    N, H, W, C = x.shape
    y = torch.empty((N, C, H, W), dtype=torch.float32, device=x.device)
    _check(lib().sc2_nhwc_bf16_to_nchw_f32(_ptr(x), _ptr(y), N, C, H, W, _stream()), 'nhwc_bf16_to_nchw_f32')
    return y


# --------------------------------------------------------------------------------------------- #
# conv
# --------------------------------------------------------------------------------------------- #
def weight_rows(cout):
    return lib().sc2_conv_weight_rows(int(cout))


def weight_pitch(k):
    return lib().sc2_conv_weight_pitch(int(k))


K_TAP_MAJOR, K_SLAB_MAJOR, K_B_TILE_MAJOR, K_B_FRAG_MAJOR = 0, 1, 2, 4   # the last two: flags OR-ed into the k order


def _pack_layout(t, k_order, fill):
    """The packed-weight LAYOUT on any tensor t [Cout, Cin, KH, KW] (any dtype): -> [Cout_pad, Kpad], padding = `fill`.
    K_TAP_MAJOR: k = (kh*KW+kw)*Cin+ci.  K_SLAB_MAJOR (Cin % 32 == 0): k = ((ci//32)*KH*KW + kh*KW+kw)*32 + ci%32."""
    cout, cin, kh, kw = t.shape
    k = cin * kh * kw
    rows, pitch = weight_rows(cout), weight_pitch(k)
    packed = torch.full((rows, pitch), fill, dtype=t.dtype, device=t.device)
    tile_major = bool(k_order & K_B_TILE_MAJOR)
    frag_major = bool(k_order & K_B_FRAG_MAJOR)
    k_order = k_order & 1
    if k_order == K_SLAB_MAJOR:
        assert cin % 32 == 0
        flat = t.reshape(cout, cin // 32, 32, kh * kw).permute(0, 1, 3, 2).reshape(cout, k)
    else:
        flat = t.permute(0, 2, 3, 1).reshape(cout, k)
    packed[:cout, :k] = flat
    if frag_major:   # [k-step][16-row tile][lane = fq*16 + frow][8]: one MFMA operand fragment = 1 KB contiguous
        rows, kpad = packed.shape
        assert rows % 16 == 0 and not tile_major
        packed = packed.reshape(rows // 16, 16, kpad // 32, 4, 8).permute(2, 0, 3, 1, 4).contiguous().reshape(rows, kpad)
    if tile_major:   # [k-slab][row][32]: same bytes, the B tile of a k-slab contiguous; kept 2-D for the shape checks
        rows, kpad = packed.shape
        packed = packed.reshape(rows, kpad // 32, 32).permute(1, 0, 2).contiguous().reshape(rows, kpad)
    return packed


def _pack_conv_weight_reference(w, k_order=K_TAP_MAJOR):
    """pack_conv_weight as the chain of layout ops it was written as (tests compare the gather form with it)."""
    return _pack_layout(w.detach().to(torch.bfloat16), k_order, 0.0)


_PACK_INDEX = {}      # (Cout, Cin, KH, KW, k_order, sub-filter key, device) -> (int32 gather map into the flat weight + one zero, shape)


def _pack_index(shape, k_order, device, sub=None):
    """Gather map of the packed layout: entry -> element of the flat [Cout, Cin, KH, KW] parameter it holds, or n (an appended zero)
    for padding.  `sub` = (rh, sh, rw, sw): the map of the DATA GRADIENT's sub-filter of one stride-parity class -- the weight seen as
    [Cin, Cout, KH, KW], taps kh = rh + sh t, kw = rw + sw u, both flipped (hip.conv2d_dgrad) -- packed straight from the parameter."""
    key = (tuple(shape), k_order, sub, str(device))
    hit = _PACK_INDEX.get(key)
    if hit is None:
        n = 1
        for v in shape:
            n *= int(v)
        idx = torch.arange(n, dtype=torch.int64, device=device).reshape(tuple(shape))
        if sub is not None:
            rh, sh, rw, sw = sub
            idx = idx.permute(1, 0, 2, 3)[:, :, rh::sh, rw::sw].flip(2, 3).contiguous()
        lay = _pack_layout(idx, k_order, n)
        hit = (lay.reshape(-1).to(torch.int32), tuple(lay.shape), bool((lay == n).any().item()))
        if len(_PACK_INDEX) > 512:
            _PACK_INDEX.clear()
        _PACK_INDEX[key] = hit
    return hit


def pack_conv_weight(w, k_order=K_TAP_MAJOR, _sub=None):
    """w: [Cout, Cin, KH, KW] (any float dtype, device) -> bf16 [Cout_pad, Kpad].

    K_TAP_MAJOR: k = (kh*KW+kw)*Cin+ci.  K_SLAB_MAJOR (Cin % 32 == 0): k = ((ci//32)*KH*KW + kh*KW+kw)*32 + ci%32.
    One cast and ONE gather through a cached index map (round 5: the chain of layout ops this replaces was five small launches per
    call, and a training step packs every trainable conv -- and every sub-filter of its data gradient -- anew)."""
    if not host_policy.pack_gather:      # A/B: the chain of layout ops
        if _sub is not None:
            rh, sh, rw, sw = _sub
            w = w.detach().permute(1, 0, 2, 3)[:, :, rh::sh, rw::sw].flip(2, 3).contiguous()
        return _pack_conv_weight_reference(w, k_order)
    idx, shape, padded = _pack_index(w.shape, k_order, w.device, _sub)
    flat = w.detach().reshape(-1).to(torch.bfloat16)
    if padded:
        flat = torch.cat([flat, flat.new_zeros(1)])
    return torch.index_select(flat, 0, idx).reshape(shape)


def conv_patch_supported(x_shape, cout, kh, kw, stride, pad, out_format=OUT_BF16_NHWC, epilogue=EPI_NONE):
    """True if this conv runs on the LDS-resident-patch kernel (weights then packed K_SLAB_MAJOR | K_B_FRAG_MAJOR)."""
    if not host_policy.conv_patch:      # A/B switch (tools/)
        return False
    (sh, sw), (ph, pw) = _pair2(stride), _pair2(pad)
    N, H, W, Cin = x_shape
    OH = (H + 2 * ph - kh) // sh + 1
    OW = (W + 2 * pw - kw) // sw + 1
    d = ConvDesc(N, H, W, Cin, cout, kh, kw, sh, sw, ph, pw, OH, OW, AOP_NONE, epilogue, out_format,
                 weight_pitch(kh * kw * Cin), weight_rows(cout), 0, 0, 0, 0, 0, 0, K_SLAB_MAJOR | K_B_FRAG_MAJOR)
    return bool(lib().sc2_conv_patch_supported(ctypes.byref(d)))


def preferred_k_order(cin, kh, kw):
    """Slab-major pays when several taps re-read overlapping pixels and the channel count allows it."""
    if host_policy.k_order_tap:      # A/B switch (tools/)
        return K_TAP_MAJOR | (K_B_TILE_MAJOR if host_policy.b_tile_major else 0)
    # measured (same box, tools/layer_times.py): +1.5 % on the 2x2 decoder convs, -4 % on the 25-tap stride-2 conv
    base = K_SLAB_MAJOR if (cin % 32 == 0 and 1 < kh * kw <= 9) else K_TAP_MAJOR
    return base | (K_B_TILE_MAJOR if host_policy.b_tile_major else 0)


def pack_conv0_weight_pairs(w):
    """First encoder conv (Cin=3, k5 s2 p2) on the pixel-pair view of the input.

    The input is stored as bf16 NHWC with channels padded 3->4, viewed as [N, H, W/2, 8]
    (8 = 2 pixels x 4 channels).  A 5-tap stride-2 row filter becomes a 3-tap stride-1 filter over
    pixel pairs: pair tap t covers original taps kw = 2t, 2t+1 (kw = 5 and channel 3 are zero).
    Returns bf16 [Cout_pad, Kpad] with k = (kh*3 + t)*8 + (dw*4 + c).
    """
    cout, cin, kh, kw = w.shape
    assert cin <= 4 and kw == 5, 'pixel-pair packing is for the 3-channel 5x5 stride-2 first conv'
    wp = torch.zeros((cout, kh, 3, 2, 4), dtype=torch.float32, device=w.device)
    wd = w.detach().float()
    for t in range(3):
        for dw in range(2):
            k = 2 * t + dw
            if k < kw:
                wp[:, :, t, dw, :cin] = wd[:, :, :, k].permute(0, 2, 1)
    k_total = kh * 3 * 8
    rows, pitch = weight_rows(cout), weight_pitch(k_total)
    packed = torch.zeros((rows, pitch), dtype=torch.bfloat16, device=w.device)
    packed[:cout, :k_total] = wp.reshape(cout, k_total).to(torch.bfloat16)
    return packed


EPI_GDN1_BWD_PRE, EPI_IGDN1_BWD_PRE, EPI_GDN1_BWD_POST = 11, 12, 13


def gdn1_bwd_gemm(x_nhwc, w_packed, epilogue, ep_x, ep_x2, beta=None, tag=None):
    """One of the two GEMMs of the GDN1 backward with the element-wise half of that backward in its epilogue
    (sc2_gdn1_bwd_gemm): -> (y, y2 or None)."""
    for t, name in ((x_nhwc, 'x'), (w_packed, 'w'), (ep_x, 'ep_x'), (ep_x2, 'ep_x2')):
        _dev(t, name)
        assert t.dtype == torch.bfloat16 and t.is_contiguous(), name
    C = x_nhwc.shape[-1]
    M = x_nhwc.numel() // C
    assert ep_x.numel() == M * C and ep_x2.numel() == M * C
    post = epilogue == EPI_GDN1_BWD_POST
    if not post:
        _dev(beta, 'beta')
        assert beta.dtype == torch.float32 and beta.is_contiguous() and beta.numel() == C
    d = ConvDesc(M, 1, 1, C, C, 1, 1, 1, 1, 0, 0, 1, 1, AOP_NONE if post else AOP_ABS, epilogue, OUT_BF16_NHWC, w_packed.shape[1],
                 w_packed.shape[0], 0, 0, 0, 0, 0, 0, K_TAP_MAJOR, 1, 1)
    y = torch.empty_like(x_nhwc)
    y2 = None if post else torch.empty_like(x_nhwc)
    with _timed(tag or 'gdn.bwd.gemm'):
        _check(lib().sc2_gdn1_bwd_gemm(ctypes.byref(d), _ptr(x_nhwc), _ptr(w_packed), _ptr(y), _ptr(y2), _ptr(ep_x), _ptr(ep_x2),
                                       _ptr(beta), _stream()), 'gdn1_bwd_gemm')
    return y, y2


def gdn1_rows_supported(x_nhwc, C):
    """True if GDN1 over C channels of this bf16 [..., C] tensor runs on the resident-row kernel (C = 96, 256 or 512, < 2 GB)."""
    return bool(host_policy.gdn_rows) and x_nhwc.dtype == torch.bfloat16 and x_nhwc.is_cuda and x_nhwc.is_contiguous() and \
        x_nhwc.shape[-1] == C and _fits32(x_nhwc.numel()) and bool(lib().sc2_gdn1_rows_supported(C))


def gdn1_rows_fwd(x_nhwc, gamma_frag, beta, inverse, tag=None):
    """y = GDN1(x) / inverse GDN1(x) for a bf16 [..., 512] tensor; gamma_frag = pack_weight_fragments(effective gamma)."""
    for t, name in ((x_nhwc, 'x'), (gamma_frag, 'gamma_frag'), (beta, 'beta')):
        _dev(t, name)
    C = x_nhwc.shape[-1]
    assert x_nhwc.dtype == torch.bfloat16 and x_nhwc.is_contiguous()
    assert gamma_frag.dtype == torch.bfloat16 and gamma_frag.is_contiguous() and tuple(gamma_frag.shape) == (C // 16, C // 32, 64, 8)
    assert beta.dtype == torch.float32 and beta.is_contiguous() and beta.numel() == C
    y = torch.empty_like(x_nhwc)
    with _timed(tag or 'gdn.rows.fwd'):
        _check(lib().sc2_gdn1_rows_fwd(_ptr(x_nhwc), _ptr(gamma_frag), _ptr(beta), _ptr(y), x_nhwc.numel() // C, C, 1 if inverse else 0,
                                       _stream()), 'gdn1_rows_fwd')
    return y


def gdn1_rows_bwd(x_nhwc, gy_nhwc, gamma_frag, gamma_t_frag, beta, inverse, tag=None, want_d_beta=False):
    """-> (d_norm, dx[, d_beta]), d_norm / dx bf16 like x: the two GEMMs of the GDN1 backward and its element-wise halves in one launch;
    want_d_beta: also the column sums of d_norm (f32 [C]; inside the launch for C = 96 / 256, a column-sum launch behind it for 512)."""
    for t, name in ((x_nhwc, 'x'), (gy_nhwc, 'gy'), (gamma_frag, 'gamma_frag'), (gamma_t_frag, 'gamma_t_frag'), (beta, 'beta')):
        _dev(t, name)
    C = x_nhwc.shape[-1]
    assert x_nhwc.dtype == torch.bfloat16 and x_nhwc.is_contiguous() and gy_nhwc.dtype == torch.bfloat16 and gy_nhwc.is_contiguous()
    assert gy_nhwc.numel() == x_nhwc.numel()
    for g in (gamma_frag, gamma_t_frag):
        assert g.dtype == torch.bfloat16 and g.is_contiguous() and tuple(g.shape) == (C // 16, C // 32, 64, 8)
    assert beta.dtype == torch.float32 and beta.is_contiguous() and beta.numel() == C
    d_norm, dx = torch.empty_like(x_nhwc), torch.empty_like(x_nhwc)
    d_beta = torch.empty((C,), dtype=torch.float32, device=x_nhwc.device) if want_d_beta else None
    with _timed(tag or 'gdn.rows.bwd'):
        _check(lib().sc2_gdn1_rows_bwd(_ptr(x_nhwc), _ptr(gy_nhwc), _ptr(gamma_frag), _ptr(gamma_t_frag), _ptr(beta), _ptr(d_norm),
                                       _ptr(dx), _ptr(d_beta), x_nhwc.numel() // C, C, 1 if inverse else 0, _stream()), 'gdn1_rows_bwd')
    return (d_norm, dx, d_beta) if want_d_beta else (d_norm, dx)


def colsum_bf16(x, C):
    """bf16 [..., C] -> f32 [C] column sums."""
    _dev(x, 'x')
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and x.shape[-1] == C
    out = torch.empty((C,), dtype=torch.float32, device=x.device)
    _check(lib().sc2_colsum_bf16(_ptr(x), x.numel() // C, C, _ptr(out), _stream()), 'colsum_bf16')
    return out


def gdn_bwd_pre(gy, x, norm, inverse):
    """First element-wise half of the five-launch GDN1 backward; gy, x, norm: bf16 [..., C] of one shape -> (d_norm bf16, dx_direct
    bf16, d_beta f32 [C]): d_norm = -gy x / norm^2 (inverse: gy x), dx_direct = gy / norm (inverse: gy norm), d_beta = column sums
    of the unrounded d_norm."""
    for t, name in ((gy, 'gy'), (x, 'x'), (norm, 'norm')):
        _dev(t, name)
        assert t.dtype == torch.bfloat16 and t.is_contiguous() and t.numel() == x.numel()
    C = x.shape[-1]
    d_norm = torch.empty_like(x)
    dxd = torch.empty_like(x)
    d_beta = torch.empty((C,), dtype=torch.float32, device=x.device)
    _check(lib().sc2_gdn_bwd_pre(_ptr(gy), _ptr(x), _ptr(norm), x.numel() // C, C, 1 if inverse else 0, _ptr(d_norm),
                                 _ptr(dxd), _ptr(d_beta), _stream()), 'gdn_bwd_pre')
    return d_norm, dxd, d_beta


def gdn_bwd_post(dx_direct, x, t):
    """Second element-wise half: dx = dx_direct + sign(x) t (t = gamma^T d_norm); bf16 tensors of one shape -> bf16."""
    for v, name in ((dx_direct, 'dx_direct'), (x, 'x'), (t, 't')):
        _dev(v, name)
        assert v.dtype == torch.bfloat16 and v.is_contiguous() and v.numel() == x.numel()
    dx = torch.empty_like(x)
    _check(lib().sc2_gdn_bwd_post(_ptr(dx_direct), _ptr(x), _ptr(t), x.numel(), _ptr(dx), _stream()), 'gdn_bwd_post')
    return dx


def gdn1_backward(gy_nhwc, x_nhwc, beta, gamma, inverse):
    """Backward of GDN1 / inverse GDN1 on the HIP kernels: returns (dx bf16 NHWC, d_beta f32 [C], d_gamma f32 [C,C]).

    beta [C] / gamma [C,C] are the effective (reparametrised) f32 tensors.  Round 5: for C = 96 and C a multiple of 128 the two
    element-wise halves ride in the epilogues of the two GEMMs (norm GEMM -> d_norm + direct term; gamma^T GEMM -> dx): nine
    passes over the [pixels, C] tensors instead of fifteen (`host_policy.gdn_bwd_fused = False`: the five-launch form, A/B)."""
    C = beta.numel()
    M = x_nhwc.numel() // C
    gy_nhwc = gy_nhwc.contiguous()
    beta = beta.detach().float().contiguous()
    if gdn1_rows_supported(x_nhwc, C):
        # C = 256 / 512: both GEMMs and both element-wise halves in ONE launch with the pixel tile's whole channel row in LDS (four passes
        # over the [pixels, C] tensors: x, g in; d_norm, dx out)
        g = gamma.detach()
        d_norm, dx, d_beta = gdn1_rows_bwd(x_nhwc, gy_nhwc, pack_weight_fragments(g), pack_weight_fragments(g.t()), beta, inverse,
                                           want_d_beta=True)
        d_gamma = conv2d_wgrad(x_nhwc, d_norm, 1, 1, 1, 0, x_abs=True).reshape(C, C)
        return dx, d_beta, d_gamma
    if host_policy.gdn_bwd_fused and (weight_rows(C) % 128 == 0 or weight_rows(C) == 96) and M < (1 << 31):
        g = gamma.detach()
        d_norm, dxd = gdn1_bwd_gemm(x_nhwc, pack_conv_weight(g.reshape(C, C, 1, 1)), EPI_IGDN1_BWD_PRE if inverse else EPI_GDN1_BWD_PRE,
                                    gy_nhwc, x_nhwc, beta, tag='gdn.bwd.pre')
        dx, _ = gdn1_bwd_gemm(d_norm, pack_conv_weight(g.t().reshape(C, C, 1, 1)), EPI_GDN1_BWD_POST, dxd, x_nhwc, tag='gdn.bwd.post')
        d_beta = colsum_bf16(d_norm, C)
        d_gamma = conv2d_wgrad(x_nhwc, d_norm, 1, 1, 1, 0, x_abs=True).reshape(C, C)
        return dx, d_beta, d_gamma
    norm = conv2d_fwd(x_nhwc, pack_conv_weight(gamma.detach().reshape(C, C, 1, 1)), C, 1, 1, 1, 0, a_op=AOP_ABS,
                      epilogue=EPI_BIAS, ep_beta=beta, tag='gdn.bwd.norm')
    d_norm, dxd, d_beta = gdn_bwd_pre(gy_nhwc, x_nhwc, norm, inverse)
    t = conv2d_fwd(d_norm, pack_conv_weight(gamma.detach().t().reshape(C, C, 1, 1)), C, 1, 1, 1, 0, tag='gdn.bwd.gT')
    dx = gdn_bwd_post(dxd, x_nhwc, t)
    d_gamma = conv2d_wgrad(x_nhwc, d_norm, 1, 1, 1, 0, x_abs=True).reshape(C, C)
    return dx, d_beta, d_gamma


def conv2d_wgrad(x_nhwc, gy_nhwc, kh, kw, stride, pad, x_abs=False):
    """Weight gradient: x bf16 [N,H,W,Cin], gy bf16 [N,OH,OW,Cout] -> f32 [Cout, Cin, KH, KW]."""
    _dev(x_nhwc, 'x')
    _dev(gy_nhwc, 'gy')
    assert x_nhwc.dtype == torch.bfloat16 and gy_nhwc.dtype == torch.bfloat16
    assert x_nhwc.is_contiguous() and gy_nhwc.is_contiguous()
    (sh, sw), (ph, pw) = _pair2(stride), _pair2(pad)
    N, H, W, Cin = x_nhwc.shape
    OH = (H + 2 * ph - kh) // sh + 1
    OW = (W + 2 * pw - kw) // sw + 1
    cout = gy_nhwc.shape[3]
    assert tuple(gy_nhwc.shape) == (N, OH, OW, cout)
    d = ConvDesc(N, H, W, Cin, cout, kh, kw, sh, sw, ph, pw, OH, OW, AOP_ABS if x_abs else AOP_NONE, 0, 0, 0, 0, 0, 0,
                 0, 0, 0, 0, 0)
    dw = torch.empty((cout, kh * kw * Cin), dtype=torch.float32, device=x_nhwc.device)
    with _timed('wgrad'):
        _check(lib().sc2_conv2d_wgrad(ctypes.byref(d), _ptr(x_nhwc), _ptr(gy_nhwc), _ptr(dw), _stream()),
               'conv2d_wgrad')
    return dw.view(cout, kh, kw, Cin).permute(0, 3, 1, 2)


def conv2d_dgrad(gy_nhwc, weight, stride, pad, in_hw, out_dtype=torch.bfloat16, cache=None):
    """Data gradient of y = conv2d(x, weight, stride, pad) on the forward implicit-GEMM kernel.

    gy_nhwc: bf16 [N,OH,OW,Cout]; weight: [Cout,Cin,KH,KW]; returns NHWC [N,H,W,Cin] (H, W = in_hw).
    A transposed convolution is, per stride-parity class (ih % s, iw % s), a stride-1 correlation of gy with the
    sub-filter of taps kh = r + s*t (r = (ih + p) % s), flipped; each class is one launch that scatters its rows
    to every s-th pixel of the gradient.  Stride 1 is the single-class case (full flip, pad k-1-p).
    `cache`: a dict owned by the caller of a FROZEN weight -- the packed sub-filters are then built once, not per step.
    """
    cout, cin, KH, KW = weight.shape
    (sh, sw), (ph, pw) = _pair2(stride), _pair2(pad)
    H, W = in_hw
    N = gy_nhwc.shape[0]
    fmt = OUT_BF16_NHWC if out_dtype == torch.bfloat16 else OUT_F32_NHWC
    gx = torch.empty((N, H, W, cin), dtype=out_dtype, device=gy_nhwc.device)
    covered_h = covered_w = 0
    wt = weight.detach().permute(1, 0, 2, 3)   # [Cin, Cout, KH, KW]
    for ch in range(sh):
        rh = (ch + ph) % sh
        khs = list(range(rh, KH, sh))
        rows = (H - ch + sh - 1) // sh if H > ch else 0
        for cw in range(sw):
            rw = (cw + pw) % sw
            kws = list(range(rw, KW, sw))
            cols = (W - cw + sw - 1) // sw if W > cw else 0
            if rows == 0 or cols == 0:
                continue
            if not khs or not kws:      # no tap reaches this parity class: its gradient is zero
                gx[:, ch::sh, cw::sw] = 0
                continue
            qh, qw = (ch + ph - rh) // sh, (cw + pw - rw) // sw
            pad_h, pad_w = len(khs) - 1 - qh, len(kws) - 1 - qw
            if pad_h < 0 or pad_w < 0:
                raise Sc2Error('conv2d_dgrad: unsupported geometry k={} s={} p={}'.format((KH, KW), (sh, sw), (ph, pw)))
            win = (sh == 1 and sw == 1 and out_dtype == torch.bfloat16 and pad_h == pad_w and gy_nhwc.is_contiguous() and
                   conv2x2_win_supported(tuple(gy_nhwc.shape), cin, len(khs), len(kws), 1, pad_h))
            # ... and a 512-channel gradient (dec.conv2: 512 -> 256, k2, p0) as two 256-channel halves of that kernel (pad 1)
            win2 = (not win and cin == 512 and pad_h == 1 and sh == 1 and sw == 1 and out_dtype == torch.bfloat16 and pad_w == 1 and
                    gy_nhwc.is_contiguous() and host_policy.dgrad_win_halves and _fits32(gx.numel()) and
                    conv2x2_win_supported(tuple(gy_nhwc.shape), 256, len(khs), len(kws), 1, 1))
            # (the packed sub-filters belong to THIS weight tensor at this version, stride and padding: a cache dict shared
            #  between layers, or kept across an optimizer step, must miss -- ADVICE r4)
            key = (ch, cw, win, win2, weight.data_ptr(), weight._version, tuple(weight.shape), (sh, sw), (ph, pw))
            packed = cache.get(key) if cache is not None else None
            if packed is None:
                # (strided SLICES, not index lists: an index list is a host tensor copied to the device per call)
                if win or win2:
                    sub = wt[:, :, rh::sh, rw::sw].flip(2, 3).contiguous()      # taps in correlation order
                    packed = (pack_conv2x2_win(sub[:256]), pack_conv2x2_win(sub[256:])) if win2 else pack_conv2x2_win(sub)
                else:   # (one gather from the parameter itself: sub-filter, flip and packed layout folded into the index map)
                    packed = pack_conv_weight(weight, K_TAP_MAJOR, _sub=(rh, sh, rw, sw))
                if cache is not None:
                    cache[key] = packed
            if sh == 1 and sw == 1:
                if win2:     # (1.07 ms on the 256-row tile kernel at bs 256)
                    conv2x2_win_fwd(gy_nhwc, packed[0], 1, tag='dgrad', out=gx, channel0=0)
                    conv2x2_win_fwd(gy_nhwc, packed[1], 1, tag='dgrad', out=gx, channel0=256)
                    continue
                if win:
                    # the decoder's last conv (256 -> 256, k2, p1): its data gradient is the k2 p0 conv of the first window-plane
                    # geometry (1.16 ms on the tile kernel at bs 256, 0.37 here)
                    gx = conv2x2_win_fwd(gy_nhwc, packed, pad_h, tag='dgrad')
                    continue
                conv2d_fwd(gy_nhwc, packed, cin, len(khs), len(kws), 1, (pad_h, pad_w), out_format=fmt, out=gx,
                           tag='dgrad')
            else:
                conv2d_fwd(gy_nhwc, packed, cin, len(khs), len(kws), 1, (pad_h, pad_w), out_format=fmt, tag='dgrad',
                           scatter=(rows, cols, gx, sh, sw, ch, cw))
    return gx


ParityClass = collections.namedtuple('ParityClass', 'off_h off_w khs kws pad_h pad_w sub')


def deconv_parity_classes(weight, stride, padding):
    """A transposed convolution as stride-1 correlations, one per stride-parity class of the output (device-free: plain torch on
    whatever device `weight` is).  weight: ConvTranspose2d's [Cin, Cout, KH, KW]; stride, padding: (h, w).  Output pixel
    (off_h + sh * r, off_w + sw * c) of class (off_h, off_w) is the correlation of the input, zero-padded by (pad_h, pad_w) at the
    top / left and as far as needed at the bottom / right, with `sub` [Cout, Cin, len(khs), len(kws)]: the taps khs x kws of the
    filter that reach the class, flipped, at row r / column c.  A class has ceil((OH - off_h) / sh) rows.
    -> [ParityClass(off_h, off_w, khs, kws, pad_h, pad_w, sub)], sh * sw entries."""
    KH, KW = int(weight.shape[2]), int(weight.shape[3])
    sh, sw = stride
    ph, pw = padding
    wt = weight.detach().permute(1, 0, 2, 3)   # [out, in, kh, kw]: rows = output channels
    classes = []
    for ch in range(sh):
        rh = (ch + ph) % sh
        khs = list(range(rh, KH, sh))
        for cw in range(sw):
            rw = (cw + pw) % sw
            kws = list(range(rw, KW, sw))
            if not khs or not kws:
                raise Sc2Error('HipConvTranspose2d: a stride-parity class without taps (k={} s={} p={})'
                               .format((KH, KW), (sh, sw), (ph, pw)))
            qh, qw = (ch + ph - rh) // sh, (cw + pw - rw) // sw
            pad_h, pad_w = len(khs) - 1 - qh, len(kws) - 1 - qw
            if pad_h < 0 or pad_w < 0:
                raise Sc2Error('HipConvTranspose2d: unsupported geometry k={} s={} p={}'.format((KH, KW), (sh, sw), (ph, pw)))
            sub = wt[:, :, khs][:, :, :, kws].flip(2, 3).contiguous()
            classes.append(ParityClass(ch, cw, khs, kws, pad_h, pad_w, sub))
    return classes


def conv_fused_gdn_supported(x_shape, cout, kh, kw, stride, pad, out_format=OUT_BF16_NHWC):
    """Non-zero if conv + GDN1 runs as ONE launch (EPI_FUSED_GDN / EPI_FUSED_IGDN) for this geometry (x_shape =
    [N,H,W,Cin]): 1 = ep_x takes GDN1.effective()'s packed-row gamma, 2 = GDN1.effective_fragments()'s."""
    (sh, sw), (ph, pw) = _pair2(stride), _pair2(pad)
    N, H, W, Cin = x_shape
    OH = (H + 2 * ph - kh) // sh + 1
    OW = (W + 2 * pw - kw) // sw + 1
    d = ConvDesc(N, H, W, Cin, cout, kh, kw, sh, sw, ph, pw, OH, OW, AOP_NONE, EPI_FUSED_GDN, out_format,
                 weight_pitch(kh * kw * Cin), weight_rows(cout), 0, 0, 0, 0, 0, 0, K_TAP_MAJOR)
    return int(lib().sc2_conv_fused_gdn_supported(ctypes.byref(d)))   # 0 no, 1 packed-row gamma, 2 fragment-major gamma


def conv2d_fwd(x_nhwc, w_packed, cout, kh, kw, stride, pad, a_op=AOP_NONE, epilogue=EPI_NONE,
               out_format=OUT_BF16_NHWC, ep_x=None, ep_beta=None, out=None, tag=None, scatter=None,
               k_order=K_TAP_MAJOR, dilation=1):
    """x_nhwc: bf16 [N,H,W,Cin]; returns the output tensor.

    out_format OUT_BF16_NHWC -> bf16 [N,OH,OW,Cout]; OUT_F32_NCHW -> f32 [N,Cout,OH,OW];
    OUT_F32_NHWC -> f32 [N,OH,OW,Cout].  stride / pad / dilation: int or (h, w) (dilation > 1: Cout > 96, plain epilogues).
    """
    _dev(x_nhwc, 'x')
    _dev(w_packed, 'w_packed')
    assert x_nhwc.dtype == torch.bfloat16 and x_nhwc.dim() == 4 and x_nhwc.is_contiguous()
    assert w_packed.dtype == torch.bfloat16 and w_packed.is_contiguous()
    (sh, sw), (ph, pw), (dh, dw) = _pair2(stride), _pair2(pad), _pair2(dilation)
    N, H, W, Cin = x_nhwc.shape
    OH = (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1
    OW = (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    sc = (0, 0, 0, 0, 0, 0)
    if scatter is not None:   # (OH, OW, out tensor [N,out_H,out_W,cout], stride_h, stride_w, off_h, off_w)
        OH, OW, out, s_h, s_w, o_h, o_w = scatter
        assert out.dtype == (torch.bfloat16 if out_format == OUT_BF16_NHWC else torch.float32) and out.is_contiguous()
        assert out.shape[0] == N and out.shape[3] == cout
        sc = (out.shape[1], out.shape[2], s_h, s_w, o_h, o_w)
    d = ConvDesc(N, H, W, Cin, cout, kh, kw, sh, sw, ph, pw, OH, OW, a_op, epilogue, out_format,
                 w_packed.shape[1], w_packed.shape[0], *(sc + (k_order, dh, dw)))
    if out is None:
        if out_format == OUT_BF16_NHWC:
            out = torch.empty((N, OH, OW, cout), dtype=torch.bfloat16, device=x_nhwc.device)
        elif out_format == OUT_F32_NCHW:
            out = torch.empty((N, cout, OH, OW), dtype=torch.float32, device=x_nhwc.device)
        elif out_format == OUT_I32_NCHW_SYM:
            out = torch.empty((N, cout, OH, OW), dtype=torch.int32, device=x_nhwc.device)
        else:
            out = torch.empty((N, OH, OW, cout), dtype=torch.float32, device=x_nhwc.device)
    if ep_x is not None:
        _dev(ep_x, 'ep_x')
        assert ep_x.dtype == torch.bfloat16 and ep_x.is_contiguous()
        if epilogue in (EPI_FUSED_GDN, EPI_FUSED_IGDN):   # ep_x carries the gamma matrix (packed rows or fragments)
            assert tuple(ep_x.shape) in ((weight_rows(cout), weight_pitch(cout)), (cout // 16, cout // 32, 64, 8))
        else:
            assert ep_x.numel() == N * OH * OW * cout
    if ep_beta is not None:
        _dev(ep_beta, 'ep_beta')
        assert ep_beta.dtype == torch.float32 and ep_beta.is_contiguous() and ep_beta.numel() == cout
    with _timed(tag or 'conv{}x{}_{}to{}'.format(kh, kw, Cin, cout)):
        _check(lib().sc2_conv2d_fwd(ctypes.byref(d), _ptr(x_nhwc), _ptr(w_packed), _ptr(out), _ptr(ep_x),
                                    _ptr(ep_beta), _stream()), 'conv2d_fwd')
    return out


def conv2x2_gdn512_supported(cin, cout, kh, kw, stride, pad):
    """True if Conv2d(cin -> 512, k2, s1, p1) followed by a 512-channel GDN1 runs as the single fused launch."""
    (sh, sw), (ph, pw) = _pair2(stride), _pair2(pad)
    return sh == sw and ph == pw and bool(lib().sc2_conv2x2_gdn512_supported(cin, cout, kh, kw, sh, ph))


def conv0_gdn96_supported(x_pairs_shape, cout):
    """True if the pixel-pair first conv + GDN1(96) runs as the single persistent launch (any width: 112-pixel output
    segments)."""
    if not host_policy.conv0_fused:      # A/B switch (tools/)
        return False
    return len(x_pairs_shape) == 4 and bool(lib().sc2_conv0_gdn96_supported(x_pairs_shape[3], cout, x_pairs_shape[2]))


def conv0_gdn96_fwd(x_pairs, w_frag, gamma_frag, beta, inverse=False, tag=None, want_t=False):
    """x_pairs bf16 [N,H,W/2,8] -> bf16 NHWC [N,(H-1)//2+1,W/2,96]; w_frag / gamma_frag: pack_weight_fragments of the
    pair-packed weights [96,128] and of the effective gamma [96,96]."""
    for t, name in ((x_pairs, 'x_pairs'), (w_frag, 'w_frag'), (gamma_frag, 'gamma_frag'), (beta, 'beta')):
        _dev(t, name)
    assert x_pairs.dtype == torch.bfloat16 and x_pairs.dim() == 4 and x_pairs.is_contiguous() and x_pairs.shape[3] == 8
    N, H, WP, _ = x_pairs.shape
    assert w_frag.dtype == torch.bfloat16 and w_frag.is_contiguous() and tuple(w_frag.shape) == (6, 4, 64, 8)
    assert gamma_frag.dtype == torch.bfloat16 and gamma_frag.is_contiguous() and tuple(gamma_frag.shape) == (6, 3, 64, 8)
    assert beta.dtype == torch.float32 and beta.is_contiguous() and beta.numel() == 96
    out = torch.empty((N, (H - 1) // 2 + 1, WP, 96), dtype=torch.bfloat16, device=x_pairs.device)
    t = torch.empty_like(out) if want_t else None        # (training: the conv output in front of the GDN)
    with _timed(tag or 'conv0_gdn96'):
        _check(lib().sc2_conv0_gdn96_fwd(_ptr(x_pairs), _ptr(w_frag), _ptr(gamma_frag), _ptr(beta), _ptr(out), _ptr(t), N, H, WP,
                                         1 if inverse else 0, _stream()), 'conv0_gdn96_fwd')
    return (out, t) if want_t else out


def conv0_gdn96_nchw_fwd(x_nchw, w_frag, gamma_frag, beta, inverse=False, tag=None):
    """The same launch on the f32 NCHW image batch [N,3,H,W] itself (W even): the colour planes are read in place and rounded
    to bf16 as they are staged -- no layout pass, bit-identical to nchw_f32_to_nhwc_bf16(x, 4) + conv0_gdn96_fwd."""
    for t, name in ((x_nchw, 'x_nchw'), (w_frag, 'w_frag'), (gamma_frag, 'gamma_frag'), (beta, 'beta')):
        _dev(t, name)
    assert x_nchw.dtype == torch.float32 and x_nchw.dim() == 4 and x_nchw.is_contiguous() and x_nchw.shape[1] == 3
    N, _, H, W = x_nchw.shape
    assert W % 2 == 0
    assert w_frag.dtype == torch.bfloat16 and w_frag.is_contiguous() and tuple(w_frag.shape) == (6, 4, 64, 8)
    assert gamma_frag.dtype == torch.bfloat16 and gamma_frag.is_contiguous() and tuple(gamma_frag.shape) == (6, 3, 64, 8)
    assert beta.dtype == torch.float32 and beta.is_contiguous() and beta.numel() == 96
    out = torch.empty((N, (H - 1) // 2 + 1, W // 2, 96), dtype=torch.bfloat16, device=x_nchw.device)
    with _timed(tag or 'conv0_gdn96'):
        _check(lib().sc2_conv0_gdn96_nchw_fwd(_ptr(x_nchw), _ptr(w_frag), _ptr(gamma_frag), _ptr(beta), _ptr(out), N, H, W,
                                              1 if inverse else 0, _stream()), 'conv0_gdn96_nchw_fwd')
    return out


def conv2_gdn48_supported(x_shape, cout, kh, kw, stride, pad):
    """True if this conv + GDN1(48) runs as the persistent weights-in-registers launch (96 -> 48, k5 s2 p2, W = 112)."""
    if not host_policy.conv2_fused:      # A/B switch (tools/)
        return False
    (sh, sw), (ph, pw) = _pair2(stride), _pair2(pad)
    return (len(x_shape) == 4 and (kh, kw, sh, sw, ph, pw) == (5, 5, 2, 2, 2, 2) and
            bool(lib().sc2_conv2_gdn48_supported(x_shape[3], cout, x_shape[2])))


def conv2_gdn48_fwd(x_nhwc, w_frag, gamma_frag, beta, inverse=False, tag=None, want_t=False):
    """x bf16 [N,H,W,96] -> bf16 NHWC [N,(H-1)//2+1,(W-1)//2+1,48] (W = 112: the static geometry of the 224 x 224 operating point;
    any other width: 56-column output segments); w_frag: pack_conv_weight(w, K_SLAB_MAJOR | K_B_FRAG_MAJOR);
    gamma_frag: pack_weight_fragments of the effective gamma zero-padded to [48, 64]."""
    for t, name in ((x_nhwc, 'x'), (w_frag, 'w_frag'), (gamma_frag, 'gamma_frag'), (beta, 'beta')):
        _dev(t, name)
    assert x_nhwc.dtype == torch.bfloat16 and x_nhwc.dim() == 4 and x_nhwc.is_contiguous() and x_nhwc.shape[3] == 96
    N, H, W, _ = x_nhwc.shape
    assert w_frag.dtype == torch.bfloat16 and w_frag.is_contiguous() and tuple(w_frag.shape) == (48, weight_pitch(2400))
    assert gamma_frag.dtype == torch.bfloat16 and gamma_frag.is_contiguous() and tuple(gamma_frag.shape) == (3, 2, 64, 8)
    assert beta.dtype == torch.float32 and beta.is_contiguous() and beta.numel() == 48
    out = torch.empty((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 48), dtype=torch.bfloat16, device=x_nhwc.device)
    t = torch.empty_like(out) if want_t else None        # (training: the conv output in front of the GDN)
    with _timed(tag or 'conv2_gdn48'):
        _check(lib().sc2_conv2_gdn48_fwd(_ptr(x_nhwc), _ptr(w_frag), _ptr(gamma_frag), _ptr(beta), _ptr(out), _ptr(t), N, H, W,
                                         1 if inverse else 0, _stream()), 'conv2_gdn48_fwd')
    return (out, t) if want_t else out


def avgpool_nhwc(x_nhwc, want_f32=True, want_bf16=False):
    """bf16 NHWC [N,H,W,C] -> (mean over H,W as f32 [N,C] or None, the same rounded to bf16 [N,C] or None)."""
    _dev(x_nhwc, 'x')
    assert x_nhwc.dtype == torch.bfloat16 and x_nhwc.dim() == 4 and x_nhwc.is_contiguous()
    N, H, W, C = x_nhwc.shape
    f32 = torch.empty((N, C), dtype=torch.float32, device=x_nhwc.device) if want_f32 else None
    b16 = torch.empty((N, C), dtype=torch.bfloat16, device=x_nhwc.device) if want_bf16 else None
    with _timed('avgpool'):
        _check(lib().sc2_avgpool_nhwc(_ptr(x_nhwc), _ptr(f32), _ptr(b16), N, H * W, C, _stream()), 'avgpool_nhwc')
    return f32, b16


def maxpool_nhwc(x_nhwc, kernel, stride, pad, tag=None):
    """nn.MaxPool2d (floor mode) on a bf16 NHWC map [N,H,W,C], C % 8 == 0 -> [N,OH,OW,C]; bit-identical to torch's."""
    _dev(x_nhwc, 'x')
    assert x_nhwc.dtype == torch.bfloat16 and x_nhwc.dim() == 4 and x_nhwc.is_contiguous()
    N, H, W, C = x_nhwc.shape
    (kh, kw), (sh, sw), (ph, pw) = [_pair2(v) for v in (kernel, stride, pad)]
    out = torch.empty((N, (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1, C), dtype=torch.bfloat16, device=x_nhwc.device)
    with _timed(tag or 'maxpool'):
        _check(lib().sc2_maxpool_nhwc(_ptr(x_nhwc), _ptr(out), N, H, W, C, kh, kw, sh, sw, ph, pw, _stream()), 'maxpool_nhwc')
    return out


def maxpool_affine_relu_nhwc(x_nhwc, a, b, kernel, stride, pad, tag=None):
    """nn.MaxPool2d (floor mode) + a per-channel affine (an eval-mode BatchNorm2d: a, b f32 [C]) + ReLU on a bf16 NHWC map
    [N,H,W,C], C % 8 == 0 -> [N,OH,OW,C]: relu(fma(a_c, max, b_c)) in f32, rounded to bf16 once.  The affine follows the max."""
    _dev(x_nhwc, 'x')
    assert x_nhwc.dtype == torch.bfloat16 and x_nhwc.dim() == 4 and x_nhwc.is_contiguous()
    N, H, W, C = x_nhwc.shape
    for t in (_dev(a, 'a'), _dev(b, 'b')):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == C
    (kh, kw), (sh, sw), (ph, pw) = [_pair2(v) for v in (kernel, stride, pad)]
    out = torch.empty((N, (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1, C), dtype=torch.bfloat16, device=x_nhwc.device)
    with _timed(tag or 'maxpool_affine_relu'):
        _check(lib().sc2_maxpool_affine_relu_nhwc(_ptr(x_nhwc), _ptr(out), _ptr(a), _ptr(b), N, H, W, C, kh, kw, sh, sw, ph, pw, _stream()),
               'maxpool_affine_relu_nhwc')
    return out


def avgpool2d_nhwc(x_nhwc, kernel, stride, tag=None):
    """nn.AvgPool2d(kernel, stride) without padding on a bf16 NHWC map [N,H,W,C], C % 8 == 0 -> [N,OH,OW,C] (f32 sum in window
    order, times 1 / kernel^2, rounded once)."""
    _dev(x_nhwc, 'x')
    assert x_nhwc.dtype == torch.bfloat16 and x_nhwc.dim() == 4 and x_nhwc.is_contiguous()
    N, H, W, C = x_nhwc.shape
    kernel, stride = int(kernel), int(stride)
    if not (0 < kernel <= min(H, W) and stride > 0):
        raise ValueError('avgpool2d_nhwc: kernel {} / stride {} on a {}x{} map'.format(kernel, stride, H, W))
    out = torch.empty((N, (H - kernel) // stride + 1, (W - kernel) // stride + 1, C), dtype=torch.bfloat16, device=x_nhwc.device)
    with _timed(tag or 'avgpool2d'):
        _check(lib().sc2_avgpool2d_nhwc(_ptr(x_nhwc), _ptr(out), N, H, W, C, kernel, stride, _stream()), 'avgpool2d_nhwc')
    return out


# --------------------------------------------------------------------------------------------- #
# CR+BQ baseline: 8-bit affine quantizer (csrc/bq.hip)
# --------------------------------------------------------------------------------------------- #
def bq_quantize(x, per_sample=False, tag=None):
    """torchdistill's `quantize_tensor(x, 8)` on the device.  x: f32, any shape (made contiguous) -> (q u8 like x, scale f32 [S],
    zero_point i32 [S], status i32 [S]) with S = 1 (the whole tensor, the reference's behaviour) or, `per_sample`, S = x.shape[0]
    (one scale per image).  status bit 1: the reference would raise ValueError (a NaN, or an all-zero segment).  Nothing here
    synchronises: the four results are device tensors."""
    _dev(x, 'x')
    assert x.dtype == torch.float32 and x.numel() > 0
    x = x.contiguous()
    assert not per_sample or x.dim() >= 1
    n_seg = int(x.shape[0]) if per_sample else 1
    n_per_seg = x.numel() // n_seg
    q = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    scale = torch.empty(n_seg, dtype=torch.float32, device=x.device)
    zs = torch.empty((2, n_seg), dtype=torch.int32, device=x.device)    # one buffer: bq_read_params brings both in one copy
    zero_point, status = zs[0], zs[1]
    partial = torch.empty(int(lib().sc2_bq_partial_len(n_seg, n_per_seg)), dtype=torch.float32, device=x.device)
    with _timed(tag or 'bq.quantize'):
        _check(lib().sc2_bq_quantize(_ptr(x), _ptr(q), _ptr(scale), _ptr(zero_point), _ptr(status), _ptr(partial), n_seg, n_per_seg,
                                     _stream()), 'bq_quantize')
    return q, scale, zero_point, status


def bq_read_params(zero_point, status):
    """(zero points, statuses) of one `bq_quantize` call as Python lists: one device-to-host copy (the call's only synchronisation)"""
    base = zero_point._base
    if base is None or base is not status._base or base.shape != (2, zero_point.numel()):
        base = torch.stack([zero_point, status])
    host = base.tolist()
    return host[0], host[1]


def _bq_params(q, scale, zero_point):
    """scale (f32 tensor, 0-dim or [S]) and zero_point (int, or integer tensor [S]) as device arrays beside q: (scale, zp, S)"""
    scale = _dev(scale, 'scale').detach().reshape(-1).to(torch.float32).contiguous()
    if isinstance(zero_point, torch.Tensor):
        zp = zero_point.to(device=q.device, dtype=torch.int32).reshape(-1).contiguous()
    else:       # a Python int (the reference's form): a fill launch, no copy from the host
        zp = torch.full((1,), int(zero_point), dtype=torch.int32, device=q.device)
    if scale.numel() != zp.numel() or scale.numel() not in (1, q.shape[0] if q.dim() else 1):
        raise ValueError('bq_dequantize: {} scales and {} zero points for codes of shape {}'.format(
            scale.numel(), zp.numel(), tuple(q.shape)))
    return scale, zp, scale.numel()


def bq_dequantize(q, scale, zero_point, out_format=OUT_F32_NCHW, affine=None, relu=False, cpad=None, tag=None):
    """torchdistill's `dequantize_tensor`: scale * (q.float() - zero_point), scale and zero point read from device memory.
    scale: f32 tensor, 0-dim / [1] (per tensor) or [q.shape[0]] (per image); zero_point: int or integer tensor likewise.
    out_format OUT_F32_NCHW -> f32 like q (any shape).  OUT_BF16_NHWC (q: u8 [N,C,H,W]) -> bf16 [N,H,W,cpad] with channels zero-padded
    to `cpad` (default: the next multiple of 8), after the optional `affine` = (a, b) f32 [C] and `relu`: relu(fma(a, v, b))."""
    _dev(q, 'q')
    assert q.dtype == torch.uint8 and q.numel() > 0
    q = q.contiguous()
    scale, zp, n_seg = _bq_params(q, scale, zero_point)
    if out_format == OUT_F32_NCHW:
        assert affine is None and not relu
        y = torch.empty(q.shape, dtype=torch.float32, device=q.device)
        with _timed(tag or 'bq.dequantize'):
            _check(lib().sc2_bq_dequantize(_ptr(q), _ptr(scale), _ptr(zp), _ptr(y), n_seg, q.numel() // n_seg, _stream()), 'bq_dequantize')
        return y
    assert out_format == OUT_BF16_NHWC and q.dim() == 4
    N, C, H, W = q.shape
    cpad = (C + 7) // 8 * 8 if cpad is None else int(cpad)
    a = b = None
    if affine is not None:
        a, b = affine
        for t in (_dev(a, 'a'), _dev(b, 'b')):
            assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == C
    y = torch.empty((N, H, W, cpad), dtype=torch.bfloat16, device=q.device)
    with _timed(tag or 'bq.dequantize'):
        _check(lib().sc2_bq_dequantize_nhwc(_ptr(q), _ptr(scale), _ptr(zp), 1 if n_seg > 1 else 0, _ptr(a), _ptr(b),
                                            1 if relu else 0, _ptr(y), N, C, H, W, cpad, _stream()), 'bq_dequantize_nhwc')
    return y


# --------------------------------------------------------------------------------------------- #
# detection tail: non-maximum suppression and multi-level RoIAlign (csrc/detect.hip)
# --------------------------------------------------------------------------------------------- #
def nms_sorted(boxes, groups, iou_threshold, keep=None, tag=None):
    """Greedy NMS of boxes that are ALREADY in processing order.  boxes: f32 [n,4] (x1, y1, x2, y2), groups: i32 [n] (boxes of
    different groups never suppress each other), n <= NMS_MAX_BOXES -> (keep u8 [n] in the same order, count i32 [1]), both on the
    device; nothing synchronises.  `keep`: a caller's u8 [n] buffer to write into.  n == 0 launches nothing."""
    _dev(boxes, 'boxes')
    _dev(groups, 'groups')
    assert boxes.dtype == torch.float32 and boxes.dim() == 2 and boxes.shape[1] == 4 and boxes.is_contiguous()
    n = int(boxes.shape[0])
    assert groups.dtype == torch.int32 and groups.shape == (n,) and groups.is_contiguous()
    if keep is None:
        keep = torch.empty(n, dtype=torch.uint8, device=boxes.device)
    assert keep.dtype == torch.uint8 and keep.shape == (n,) and keep.is_contiguous() and keep.device == boxes.device
    count = torch.empty(1, dtype=torch.int32, device=boxes.device)
    if n == 0:
        return keep, count.zero_()
    if n > NMS_MAX_BOXES:
        raise ValueError('nms_sorted: {} boxes in one call (at most {}); batched_nms splits by group'.format(n, NMS_MAX_BOXES))
    ws = torch.empty(int(lib().sc2_nms_ws_bytes(n)), dtype=torch.uint8, device=boxes.device)
    with _timed(tag or 'nms'):
        _check(lib().sc2_nms(_ptr(boxes), _ptr(groups), n, float(iou_threshold), _ptr(keep), _ptr(count), _ptr(ws), _stream()), 'nms')
    return keep, count


def batched_nms(boxes, scores, idxs, iou_threshold, tag=None):
    """torchvision's `batched_nms` in its "vanilla" form: greedy NMS within each value of `idxs`, -> int64 indices of the kept boxes
    in descending score order (ties: the lower index first -- a STABLE descending sort decides the processing order).
    torchvision's other form adds `idx * (max coordinate + 1)` to every box and runs one plain NMS; that perturbs the f32
    coordinates (the offsets are rounded into them), so its decisions near the threshold are not those of the definition: not
    built here.
    More than NMS_MAX_BOXES boxes are split by group into several calls (groups are independent: the result is unchanged); a
    single group above the cap raises ValueError.  The returned index list has a data-dependent length: one synchronising
    `nonzero`, as in torchvision (plus one `unique` where the input has to be split)."""
    _dev(boxes, 'boxes')
    n = int(boxes.shape[0])
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=boxes.device)
    order = torch.sort(scores, descending=True, stable=True)[1]
    b = boxes.detach().to(torch.float32)[order].contiguous()
    g = idxs[order].to(torch.int32).contiguous()
    if n <= NMS_MAX_BOXES:
        keep, _ = nms_sorted(b, g, iou_threshold, tag=tag)
        return order[keep.bool()]
    values, counts = torch.unique(g, return_counts=True)
    values, counts = values.tolist(), counts.tolist()
    if max(counts) > NMS_MAX_BOXES:
        raise ValueError('batched_nms: a single group holds {} boxes (at most {} per group)'.format(max(counts), NMS_MAX_BOXES))
    keep = torch.zeros(n, dtype=torch.bool, device=boxes.device)
    i = 0
    while i < len(values):       # consecutive groups up to the cap per call
        j, total = i, 0
        while j < len(values) and total + counts[j] <= NMS_MAX_BOXES:
            total += counts[j]
            j += 1
        sel = ((g >= values[i]) & (g <= values[j - 1])).nonzero().squeeze(1)       # ascending: the processing order is kept
        part, _ = nms_sorted(b[sel].contiguous(), g[sel].contiguous(), iou_threshold, tag=tag)
        keep[sel] = part.bool()
        i = j
    return order[keep]


def nms(boxes, scores, iou_threshold, tag=None):
    """torchvision's `nms`: `batched_nms` with every box in one group (at most NMS_MAX_BOXES boxes)."""
    return batched_nms(boxes, scores, torch.zeros(boxes.shape[0], dtype=torch.int32, device=boxes.device), iou_threshold, tag=tag)


def roi_align(feats_nhwc, scales, rois, levels, output_size, sampling_ratio, out=None, tag=None):
    """Multi-level RoIAlign, torchvision's aligned=False semantics (include/sc2_bottleneck.h: sc2_roi_align).
    feats_nhwc: up to ROI_MAX_LEVELS maps [N,H_l,W_l,C], contiguous, all f32 or all bf16, C % 8 == 0; scales: one float per map
    (image pixels -> map pixels); rois: f32 [K,5] (image index, x1, y1, x2, y2); levels: i32 [K], the map each RoI is pooled from
    -> f32 [K,C,P,P].  A RoI whose level or image index does not exist comes back as NaN."""
    feats_nhwc = list(feats_nhwc)
    if not 1 <= len(feats_nhwc) <= ROI_MAX_LEVELS or len(scales) != len(feats_nhwc):
        raise ValueError('roi_align: {} maps, {} scales (1..{} of each)'.format(len(feats_nhwc), len(scales), ROI_MAX_LEVELS))
    f0 = _dev(feats_nhwc[0], 'feats')
    N, C = int(f0.shape[0]), int(f0.shape[3])
    lv = RoiLevels()
    for l, (f, sc) in enumerate(zip(feats_nhwc, scales)):
        _dev(f, 'feats')
        assert f.dim() == 4 and f.is_contiguous() and f.dtype == f0.dtype and f.shape[0] == N and f.shape[3] == C and f.device == f0.device
        lv.level[l].data, lv.level[l].H, lv.level[l].W, lv.level[l].spatial_scale = f.data_ptr(), int(f.shape[1]), int(f.shape[2]), float(sc)
    assert f0.dtype in (torch.float32, torch.bfloat16)
    _dev(rois, 'rois')
    _dev(levels, 'levels')
    K, P = int(rois.shape[0]), int(output_size)
    assert rois.dtype == torch.float32 and rois.shape == (K, 5) and rois.is_contiguous()
    assert levels.dtype == torch.int32 and levels.shape == (K,) and levels.is_contiguous()
    if out is None:
        out = torch.empty((K, C, P, P), dtype=torch.float32, device=f0.device)
    assert out.dtype == torch.float32 and out.shape == (K, C, P, P) and out.is_contiguous() and out.device == f0.device
    with _timed(tag or 'roi_align'):
        _check(lib().sc2_roi_align(lv, len(feats_nhwc), N, C, 1 if f0.dtype == torch.bfloat16 else 0, _ptr(rois), _ptr(levels), K, P,
                                   int(sampling_ratio), _ptr(out), _stream()), 'roi_align')
    return out


def roi_align_backward(grad_out, map_sizes, scales, rois, levels, n_images, sampling_ratio, out=None, tag=None):
    """The adjoint of `roi_align` with respect to f32 maps (include/sc2_bottleneck.h: sc2_roi_align_backward).
    grad_out: f32 [K,C,P,P] contiguous; map_sizes: (H_l, W_l) per level; scales, rois f32 [K,5], levels i32 [K], sampling_ratio: the
    forward call's; n_images: N -> a list of f32 [N,H_l,W_l,C] gradients, every element written (zeros where nothing lands), the
    same bits on every call.  `out`: the caller's list of such tensors to write into.  A RoI whose level or image index does not
    exist contributes nothing.  The RoIs are binned by (level, image) with torch ops on the device (a stable sort: ascending index
    within a bin); nothing synchronises."""
    _dev(grad_out, 'grad_out')
    map_sizes = [(int(h), int(w)) for h, w in map_sizes]
    L = len(map_sizes)
    if not 1 <= L <= ROI_MAX_LEVELS or len(scales) != L:
        raise ValueError('roi_align_backward: {} maps, {} scales (1..{} of each)'.format(L, len(scales), ROI_MAX_LEVELS))
    assert grad_out.dtype == torch.float32 and grad_out.dim() == 4 and grad_out.is_contiguous() and grad_out.shape[2] == grad_out.shape[3]
    K, C, P, N = int(grad_out.shape[0]), int(grad_out.shape[1]), int(grad_out.shape[2]), int(n_images)
    dev = grad_out.device
    assert rois.dtype == torch.float32 and rois.shape == (K, 5) and rois.is_contiguous() and rois.device == dev
    assert levels.dtype == torch.int32 and levels.shape == (K,) and levels.is_contiguous() and levels.device == dev
    if out is None:
        out = [torch.empty((N, h, w, C), dtype=torch.float32, device=dev) for h, w in map_sizes]
    out = list(out)
    lv = RoiLevels()
    assert len(out) == L
    for l, (g, (h, w), sc) in enumerate(zip(out, map_sizes, scales)):
        assert g.dtype == torch.float32 and g.shape == (N, h, w, C) and g.is_contiguous() and g.device == dev
        lv.level[l].data, lv.level[l].H, lv.level[l].W, lv.level[l].spatial_scale = g.data_ptr(), h, w, float(sc)
    n_bins = L * N
    img = rois[:, 0]
    valid = (levels >= 0) & (levels < L) & (img >= 0) & (img < N)      # (a NaN image index compares false)
    key = torch.where(valid, levels.to(torch.int64) * N + img.clamp(0, max(N - 1, 0)).to(torch.int64), torch.full_like(levels, n_bins, dtype=torch.int64))
    order = torch.sort(key, stable=True)[1].to(torch.int32)
    bin_off = torch.zeros(n_bins + 2, dtype=torch.int64, device=dev)
    bin_off[1:] = torch.cumsum(torch.bincount(key, minlength=n_bins + 1), 0)
    bin_off = bin_off.to(torch.int32)
    with _timed(tag or 'roi_align_backward'):
        _check(lib().sc2_roi_align_backward(lv, L, N, C, _ptr(grad_out), _ptr(rois), _ptr(levels), _ptr(order), _ptr(bin_off), K, P,
                                            int(sampling_ratio), _stream()), 'roi_align_backward')
    return out


def box_match(gt_boxes, gt_counts, boxes, counts, low, high, allow_low_quality, out=None, want_iou=True, tag=None):
    """torchvision's `Matcher` over `box_iou` for several images in one call, without the IoU matrix (include/sc2_bottleneck.h:
    sc2_box_match).  gt_boxes: f32 [sum G_i,4]; boxes: f32 [sum A_i,4] (the candidates); gt_counts, counts: the G_i and A_i as Python
    ints (they become the offsets: increasing by construction; `gt_offsets=` / `offsets=` style lists are what the library checks).
    -> (matches i32 [sum A_i]: the gt index local to the image, -1 below `low`, -2 between the thresholds; best_iou f32 [sum A_i] or
    None with want_iou=False).  `out`: (matches, best_iou or None) buffers of the caller to write into.  Ties go to the lowest gt
    index, a NaN IoU is never the maximum, an image without gt boxes is all -1 / 0."""
    return box_match_offsets(gt_boxes, _offsets(gt_counts), boxes, _offsets(counts), low, high, allow_low_quality, out=out,
                             want_iou=want_iou, tag=tag)


def _offsets(counts):
    off = [0]
    for c in counts:
        off.append(off[-1] + int(c))
    return off


def box_match_offsets(gt_boxes, gt_offsets, boxes, offsets, low, high, allow_low_quality, out=None, want_iou=True, tag=None):
    """`box_match` with the two offset lists ([n_img + 1] Python ints each) given as they are: the library refuses lists that do not
    start at 0, that decrease or that do not end at the row counts (ValueError), before anything is launched."""
    _dev(boxes, 'boxes')
    _dev(gt_boxes, 'gt_boxes')
    assert boxes.dtype == torch.float32 and boxes.dim() == 2 and boxes.shape[1] == 4 and boxes.is_contiguous()
    assert gt_boxes.dtype == torch.float32 and gt_boxes.dim() == 2 and gt_boxes.shape[1] == 4 and gt_boxes.is_contiguous()
    assert gt_boxes.device == boxes.device and len(gt_offsets) == len(offsets) >= 1
    dev, n_img = boxes.device, len(offsets) - 1
    A, G = int(boxes.shape[0]), int(gt_boxes.shape[0])
    if out is None:
        out = (torch.empty(A, dtype=torch.int32, device=dev), torch.empty(A, dtype=torch.float32, device=dev) if want_iou else None)
    matches, best = out
    assert matches.dtype == torch.int32 and matches.shape == (A,) and matches.is_contiguous() and matches.device == dev
    assert best is None or (best.dtype == torch.float32 and best.shape == (A,) and best.is_contiguous() and best.device == dev)
    if not all(-2 ** 31 <= int(v) < 2 ** 31 for v in list(gt_offsets) + list(offsets)):
        raise ValueError('box_match: an offset does not fit 32 bits')
    g_host = (ctypes.c_int32 * (n_img + 1))(*[int(v) for v in gt_offsets])
    a_host = (ctypes.c_int32 * (n_img + 1))(*[int(v) for v in offsets])
    both = torch.tensor([int(v) for v in gt_offsets] + [int(v) for v in offsets], dtype=torch.int32).to(dev)
    longest = max([0] + [int(offsets[i + 1]) - int(offsets[i]) for i in range(n_img)])
    ws = torch.empty(max(int(lib().sc2_box_match_ws_bytes(G, max(longest, 0))) // 4, 1), dtype=torch.float32, device=dev)
    with _timed(tag or 'box_match'):
        _check(lib().sc2_box_match(_ptr(gt_boxes), _ptr(both[:n_img + 1]), _ptr(boxes), _ptr(both[n_img + 1:]), g_host, a_host, n_img, G, A,
                                   float(low), float(high), 1 if allow_low_quality else 0, _ptr(matches), _ptr(best), _ptr(ws),
                                   _stream()), 'box_match')
    return matches, best


DetPostResult = collections.namedtuple('DetPostResult', ['boxes', 'scores', 'labels', 'count_status', 'candidates'])
_det_post_ws = dict()          # (device index, stream, bytes) -> the workspace of sc2_det_postprocess
_DET_POST_WS_KEPT = 4


def det_postprocess_ws_bytes(R, C, n, D):
    """Bytes of sc2_det_postprocess's workspace (0: dimensions outside the kernel's range)."""
    return int(lib().sc2_det_postprocess_ws_bytes(int(R), int(C), int(n), int(D)))


def _stream_workspace(cache, kept, device, n_bytes):
    """One workspace per (device, stream, size) in `cache`: the launches of a stream are ordered, so its next call may write where the
    last one read.  The `kept` most recent sizes stay."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, n_bytes)
    ws = cache.pop(key, None)
    if ws is None:
        ws = torch.empty((n_bytes,), dtype=torch.uint8, device=device)
    cache[key] = ws               # (most recent last)
    while len(cache) > kept:
        cache.pop(next(iter(cache)))
    return ws


def det_postprocess(logits, deltas, proposals, counts, image_sizes, weights, bbox_xform_clip, score_thresh, min_size, nms_thresh,
                    detections_per_img, out=None, ws=None, want_candidates=False, tag=None):
    """torchvision's `RoIHeads.postprocess_detections` for a batch in three launches (include/sc2_bottleneck.h: sc2_det_postprocess).
    logits f32 [R,C], deltas f32 [R,4C], proposals f32 [R,4], all contiguous on the device; counts: the proposals per image and
    image_sizes: (height, width) per image, as Python ints; weights: BoxCoder's four; D = detections_per_img.
    2 <= C <= DETPOST_MAX_CLASSES and 1 <= D <= DETPOST_MAX_DET (ValueError otherwise: there is no other path in this module).
    -> DetPostResult: boxes f32 [n,D,4], scores f32 [n,D], labels i64 [n,D], every slot written (zeros behind an image's detections);
    count_status i32 [2,n] -- row 0 the detections per image, row 1 the status (0, or DETPOST_OVER_CAND / DETPOST_OVER_SEG for an image
    above a cap, whose count is 0) -- one tensor so that one copy brings both to the host; nothing synchronises here.
    `out`: (boxes, scores, labels, count_status) buffers of the caller, `ws`: a uint8 workspace of det_postprocess_ws_bytes(...) bytes
    (default: cached per device, stream and size).  want_candidates: `candidates` = (scores f32 [R,C-1], boxes f32 [R,C-1,4]), stage
    A's whole table (a test hook), else None."""
    _dev(logits, 'logits')
    _dev(deltas, 'deltas')
    _dev(proposals, 'proposals')
    dev = logits.device
    R, C, n, D = int(logits.shape[0]), int(logits.shape[1]), len(counts), int(detections_per_img)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.is_contiguous()
    assert deltas.dtype == torch.float32 and deltas.shape == (R, 4 * C) and deltas.is_contiguous() and deltas.device == dev
    assert proposals.dtype == torch.float32 and proposals.shape == (R, 4) and proposals.is_contiguous() and proposals.device == dev
    assert len(image_sizes) == n and len(weights) == 4
    if not (2 <= C <= DETPOST_MAX_CLASSES and 1 <= D <= DETPOST_MAX_DET):
        raise ValueError('det_postprocess: {} classes, {} detections per image (2..{}, 1..{})'.format(C, D, DETPOST_MAX_CLASSES, DETPOST_MAX_DET))
    offsets = _offsets(counts)
    flat = offsets + [int(v) for hw in image_sizes for v in hw]
    if len(flat) != 3 * n + 1 or not all(-2 ** 31 <= v < 2 ** 31 for v in flat):
        raise ValueError('det_postprocess: image sizes are (height, width) pairs; every offset and size fits 32 bits')
    if out is None:
        out = (torch.empty((n, D, 4), dtype=torch.float32, device=dev), torch.empty((n, D), dtype=torch.float32, device=dev),
               torch.empty((n, D), dtype=torch.int64, device=dev), torch.empty((2, n), dtype=torch.int32, device=dev))
    boxes, scores, labels, count_status = out
    for t, dt, shape in ((boxes, torch.float32, (n, D, 4)), (scores, torch.float32, (n, D)), (labels, torch.int64, (n, D)),
                         (count_status, torch.int32, (2, n))):
        assert t.dtype == dt and t.shape == shape and t.is_contiguous() and t.device == dev
    n_bytes = det_postprocess_ws_bytes(R, C, n, D)
    if ws is None:
        ws = _stream_workspace(_det_post_ws, _DET_POST_WS_KEPT, dev, max(n_bytes, 16))
    assert ws.dtype == torch.uint8 and ws.is_contiguous() and ws.numel() >= n_bytes and ws.device == dev
    cand = None
    if want_candidates:
        cand = (torch.empty((R, C - 1), dtype=torch.float32, device=dev), torch.empty((R, C - 1, 4), dtype=torch.float32, device=dev))
    host = (ctypes.c_int32 * (n + 1))(*offsets)
    both = torch.tensor(flat, dtype=torch.int32).to(dev)
    with _timed(tag or 'det_postprocess'):
        _check(lib().sc2_det_postprocess(_ptr(logits), _ptr(deltas), _ptr(proposals), _ptr(both[:n + 1]), host, _ptr(both[n + 1:]), R, C, n,
                                         float(weights[0]), float(weights[1]), float(weights[2]), float(weights[3]),
                                         float(bbox_xform_clip), float(score_thresh), float(min_size), float(nms_thresh), D,
                                         _ptr(boxes), _ptr(scores), _ptr(labels), _ptr(count_status[0]), _ptr(count_status[1]),
                                         _ptr(cand[0]) if cand else None, _ptr(cand[1]) if cand else None, _ptr(ws), _stream()),
               'det_postprocess')
    return DetPostResult(boxes, scores, labels, count_status, cand)


RpnPostResult = collections.namedtuple('RpnPostResult', ['boxes', 'scores', 'count', 'candidates'])
_rpn_post_ws = dict()          # (device index, stream, bytes) -> the workspace of sc2_rpn_proposals
_RPN_POST_WS_KEPT = 4


def rpn_proposals_ws_bytes(N, L, K, P):
    """Bytes of sc2_rpn_proposals's workspace (0: dimensions outside the kernel's range)."""
    return int(lib().sc2_rpn_proposals_ws_bytes(int(N), int(L), int(K), int(P)))


def rpn_proposals_in_range(level_shapes, N, K, P):
    """Whether sc2_rpn_proposals takes these dimensions: level_shapes = [(A_l, H_l, W_l)], N images, K / P the pre- / post-NMS top-n."""
    counts = [int(a) * int(h) * int(w) for a, h, w in level_shapes]
    return (1 <= len(counts) <= RPNPOST_MAX_LEVELS and all(c >= 1 for c in counts) and 0 <= N <= 65535 and 1 <= K <= RPNPOST_MAX_PRE_NMS
            and 1 <= P <= RPNPOST_MAX_POST_NMS and sum(min(K, c) for c in counts) <= RPNPOST_MAX_KEYS and sum(counts) < RPNPOST_MAX_ANCHORS)


def rpn_proposals(objectness_levels, delta_levels, anchors, image_sizes, K, P, nms_thresh, score_thresh, min_size, weights, clip,
                  out=None, ws=None, want_candidates=False, tag=None):
    """torchvision's `RegionProposalNetwork.filter_proposals`, with the decode of the anchors it selects, for a batch in three
    launches (include/sc2_bottleneck.h: sc2_rpn_proposals).  objectness_levels / delta_levels: the RPN head's outputs, per level
    f32 [N,A_l,H_l,W_l] / [N,4 A_l,H_l,W_l], contiguous on the device and read in place; anchors: f32 [T,4], the anchors of ONE
    image in `AnchorGenerator`'s order; image_sizes: (height, width) per image, as Python ints; K / P: the pre-NMS top-n per level /
    the post-NMS top-n; weights: BoxCoder's four, clip: its bbox_xform_clip.  Dimensions outside `rpn_proposals_in_range` raise
    ValueError: there is no other path in this module.
    -> RpnPostResult: boxes f32 [N,P,4], scores f32 [N,P], every slot written (zeros behind an image's proposals), count i32 [N];
    nothing synchronises here.  `out`: (boxes, scores, count) buffers of the caller, `ws`: a uint8 workspace of
    rpn_proposals_ws_bytes(N, L, K, P) bytes (default: cached per device, stream and size).  want_candidates: `candidates` =
    (index i32 [N,L,K], scores f32 [N,L,K], boxes f32 [N,L,K,4], k i32 [N,L]), the table of the selection by rank (a test hook),
    else None."""
    L, N, K, P = len(objectness_levels), len(image_sizes), int(K), int(P)
    assert len(delta_levels) == L and len(weights) == 4
    if L < 1:
        raise ValueError('rpn_proposals: no level')
    _dev(anchors, 'anchors')
    dev = anchors.device
    shapes = []
    for o, d in zip(objectness_levels, delta_levels):
        _dev(o, 'objectness')
        _dev(d, 'deltas')
        assert o.dtype == torch.float32 and o.dim() == 4 and o.is_contiguous() and o.device == dev and int(o.shape[0]) == N
        A, H, W = (int(v) for v in o.shape[1:])
        assert d.dtype == torch.float32 and d.shape == (N, 4 * A, H, W) and d.is_contiguous() and d.device == dev
        shapes.append((A, H, W))
    if not rpn_proposals_in_range(shapes, N, K, P):
        raise ValueError('rpn_proposals: levels {}, {} images, top-n {} / {} outside the kernel\'s range (at most {} levels, {} / {}, '
                         '{} selected anchors per image)'.format(shapes, N, K, P, RPNPOST_MAX_LEVELS, RPNPOST_MAX_PRE_NMS,
                                                                 RPNPOST_MAX_POST_NMS, RPNPOST_MAX_KEYS))
    T = sum(a * h * w for a, h, w in shapes)
    assert anchors.dtype == torch.float32 and anchors.shape == (T, 4) and anchors.is_contiguous()
    flat = [int(v) for hw in image_sizes for v in hw]
    if len(flat) != 2 * N or not all(-2 ** 31 <= v < 2 ** 31 for v in flat):
        raise ValueError('rpn_proposals: image sizes are (height, width) pairs that fit 32 bits')
    if out is None:
        out = (torch.empty((N, P, 4), dtype=torch.float32, device=dev), torch.empty((N, P), dtype=torch.float32, device=dev),
               torch.empty((N,), dtype=torch.int32, device=dev))
    boxes, scores, count = out
    for t, dt, shape in ((boxes, torch.float32, (N, P, 4)), (scores, torch.float32, (N, P)), (count, torch.int32, (N,))):
        assert t.dtype == dt and t.shape == shape and t.is_contiguous() and t.device == dev
    n_bytes = rpn_proposals_ws_bytes(N, L, K, P)
    if ws is None:
        ws = _stream_workspace(_rpn_post_ws, _RPN_POST_WS_KEPT, dev, max(n_bytes, 16))
    assert ws.dtype == torch.uint8 and ws.is_contiguous() and ws.numel() >= n_bytes and ws.device == dev
    cand = None
    if want_candidates:
        cand = (torch.empty((N, L, K), dtype=torch.int32, device=dev), torch.empty((N, L, K), dtype=torch.float32, device=dev),
                torch.empty((N, L, K, 4), dtype=torch.float32, device=dev), torch.empty((N, L), dtype=torch.int32, device=dev))
    if N == 0:
        return RpnPostResult(boxes, scores, count, cand)
    obj_ptrs = (ctypes.c_void_p * L)(*[int(o.data_ptr()) for o in objectness_levels])
    del_ptrs = (ctypes.c_void_p * L)(*[int(d.data_ptr()) for d in delta_levels])
    dims = [(ctypes.c_int32 * L)(*[s[q] for s in shapes]) for q in range(3)]
    sizes = torch.tensor(flat, dtype=torch.int32).to(dev)
    hook = [_ptr(c) for c in cand] if cand else [None] * 4
    with _timed(tag or 'rpn_proposals'):
        _check(lib().sc2_rpn_proposals(obj_ptrs, del_ptrs, dims[0], dims[1], dims[2], L, _ptr(anchors), _ptr(sizes), N, K, P,
                                       float(nms_thresh), float(score_thresh), float(min_size), float(weights[0]), float(weights[1]),
                                       float(weights[2]), float(weights[3]), float(clip), _ptr(boxes), _ptr(scores), _ptr(count),
                                       hook[0], hook[1], hook[2], hook[3], _ptr(ws), _stream()), 'rpn_proposals')
    return RpnPostResult(boxes, scores, count, cand)


# --------------------------------------------------------------------------------------------- #
# segmentation tail: labels of the resized logits and confusion counts in one launch (csrc/seg.hip)
# --------------------------------------------------------------------------------------------- #
def seg_predict(logits, size, targets=None, mat=None, want_labels=True, tag=None):
    """`F.interpolate(logits, size, mode='bilinear', align_corners=False).argmax(1)` and the confusion-matrix update of
    `SegEvaluator`, in f32 on the unrounded logits, without the resized tensor (include/sc2_bottleneck.h: sc2_seg_predict).
    logits: [N,C,h,w] f32 or bf16 with any non-negative strides (NCHW, a slice, the permuted view of a padded NHWC map), C <= 64
    (more raises Sc2Error); size: (H, W); targets: int64 [N,H,W]; mat: int64 [C,C] contiguous, ADDED to where 0 <= target < C.
    -> int64 labels [N,H,W], or None with want_labels=False (then targets and mat are required)."""
    _dev(logits, 'logits')
    assert logits.dim() == 4 and logits.dtype in (torch.float32, torch.bfloat16)
    N, C, h, w = (int(v) for v in logits.shape)
    H, W = int(size[0]), int(size[1])
    if (targets is None) != (mat is None):
        raise ValueError('seg_predict: targets and mat are given together or not at all')
    if targets is None and not want_labels:
        raise ValueError('seg_predict: nothing to compute (no labels wanted, no targets and mat)')
    if targets is not None:
        _dev(targets, 'targets')
        _dev(mat, 'mat')
        assert targets.dtype == torch.int64 and targets.shape == (N, H, W) and targets.is_contiguous() and targets.device == logits.device
        assert mat.dtype == torch.int64 and mat.shape == (C, C) and mat.is_contiguous() and mat.device == logits.device
    labels = torch.empty((N, H, W), dtype=torch.int64, device=logits.device) if want_labels else None
    with _timed(tag or 'seg_predict'):
        _check(lib().sc2_seg_predict(*(_seg_logits_args(logits) + (H, W, _ptr(targets), _ptr(labels), _ptr(mat), _stream()))), 'seg_predict')
    return labels


def _seg_logits_args(logits):
    """the leading arguments of the sc2_seg_* calls: pointer, is_bf16, N, C, h, w, the four element strides, c_readable"""
    N, C, h, w = (int(v) for v in logits.shape)
    sn, sc, sh, sw = (int(v) for v in logits.stride())
    # elements readable behind every pixel's class 0: the kernel's 16-byte class loads run up to C rounded up to 8 (bf16) / 4 (f32)
    readable = C
    if sc == 1:
        vec = 8 if logits.dtype == torch.bfloat16 else 4
        last = logits.storage_offset() + (N - 1) * sn + (h - 1) * sh + (w - 1) * sw
        if last + (C + vec - 1) // vec * vec <= logits.untyped_storage().nbytes() // logits.element_size():
            readable = (C + vec - 1) // vec * vec
    return (_ptr(logits), 1 if logits.dtype == torch.bfloat16 else 0, N, C, h, w, sn, sc, sh, sw, readable)


# --------------------------------------------------------------------------------------------- #
# segmentation training loss: cross entropy of the resized logits, forward and backward, from the low-resolution map (csrc/seg_loss.hip)
# --------------------------------------------------------------------------------------------- #
SegCeForward = collections.namedtuple('SegCeForward', ['sums', 'lse', 'pixel_loss'])


def _seg_ce_check(logits, size, targets, who):
    _dev(logits, 'logits')
    _dev(targets, 'targets')
    assert logits.dim() == 4 and logits.dtype in (torch.float32, torch.bfloat16)
    N = int(logits.shape[0])
    H, W = int(size[0]), int(size[1])
    assert targets.dtype == torch.int64 and targets.shape == (N, H, W) and targets.is_contiguous() and targets.device == logits.device, who
    return N, H, W


def seg_ce_forward(logits, size, targets, ignore_index=255, want_pixel_loss=False, want_lse=True, tag=None):
    """Cross entropy of `F.interpolate(logits, size, mode='bilinear', align_corners=False)` against `targets`, in f32 on the unrounded
    logits, without the resized tensor (include/sc2_bottleneck.h: sc2_seg_ce_forward).  logits: [N,C,h,w] f32 or bf16 with any
    non-negative strides, C <= 64 (more raises Sc2Error); targets: int64 [N,H,W] contiguous.
    -> SegCeForward(sums, lse, pixel_loss): sums = 24 device bytes viewed as float64 [3] (view(torch.int64)[1:] are the number of valid
    pixels and of bad targets), lse f32 [N,H,W] (what seg_ce_backward reads) or None, pixel_loss f32 [N,H,W] (0 at skipped pixels) or
    None.  Nothing is read back."""
    N, H, W = _seg_ce_check(logits, size, targets, 'seg_ce_forward')
    dev = logits.device
    sums = torch.empty(3, dtype=torch.float64, device=dev)
    ws = torch.empty(max(int(lib().sc2_seg_ce_ws_bytes(N, H, W)), 8) // 8, dtype=torch.float64, device=dev)
    lse = torch.empty((N, H, W), dtype=torch.float32, device=dev) if want_lse else None
    pixel_loss = torch.empty((N, H, W), dtype=torch.float32, device=dev) if want_pixel_loss else None
    with _timed(tag or 'seg_ce_forward'):
        _check(lib().sc2_seg_ce_forward(*(_seg_logits_args(logits) + (H, W, _ptr(targets), int(ignore_index), _ptr(pixel_loss), _ptr(lse),
                                                                      _ptr(sums), _ptr(ws), _stream()))), 'seg_ce_forward')
    return SegCeForward(sums, lse, pixel_loss)


def seg_ce_backward(logits, size, targets, lse, sums, grad_out, ignore_index=255, reduction=SEG_CE_MEAN, out=None, tag=None):
    """The gradient of `seg_ce_forward`'s loss with respect to the low-resolution logits (include/sc2_bottleneck.h:
    sc2_seg_ce_backward): a gather, no atomics, every element written.  lse, sums: what the forward returned; grad_out: f32 device
    scalar (SEG_CE_MEAN, SEG_CE_SUM) or f32 [N,H,W] (SEG_CE_NONE); out: a tensor of the logits' shape and dtype with any non-negative
    strides, or None (then contiguous in the logits' memory format is allocated).  -> dx"""
    N, H, W = _seg_ce_check(logits, size, targets, 'seg_ce_backward')
    dev = logits.device
    for name, t in (('lse', lse), ('sums', sums), ('grad_out', grad_out)):
        _dev(t, name)
    assert lse.dtype == torch.float32 and lse.shape == (N, H, W) and lse.is_contiguous() and lse.device == dev
    assert sums.dtype == torch.float64 and sums.numel() == 3 and sums.is_contiguous() and sums.device == dev
    assert reduction in (SEG_CE_MEAN, SEG_CE_SUM, SEG_CE_NONE)
    assert grad_out.dtype == torch.float32 and grad_out.is_contiguous() and grad_out.device == dev
    assert grad_out.shape == (N, H, W) if reduction == SEG_CE_NONE else grad_out.numel() == 1
    if out is None:
        out = torch.empty_like(logits)      # (preserve_format: a permuted NHWC view gets a dense gradient of the same layout)
    assert out.shape == logits.shape and out.dtype == logits.dtype and out.device == dev and all(int(v) >= 0 for v in out.stride())
    with _timed(tag or 'seg_ce_backward'):
        _check(lib().sc2_seg_ce_backward(*(_seg_logits_args(logits) + (H, W, _ptr(targets), int(ignore_index), _ptr(lse), _ptr(sums),
                                                                       _ptr(grad_out), int(reduction), _ptr(out)) +
                                           tuple(int(v) for v in out.stride()) + (_stream(),))), 'seg_ce_backward')
    return out


# --------------------------------------------------------------------------------------------- #
# codec feature compression: a feature map through baseline JPEG, three channels per image (csrc/jpeg.hip)
# --------------------------------------------------------------------------------------------- #
JpegCodecResult = collections.namedtuple('JpegCodecResult', ['recon', 'sizes', 'status', 'extrema', 'meta', 'bytes', 'slot_bytes'])


def jpeg_max_bytes(mode, H, W):
    """Upper bound of one image's entropy-coded segment (mode: JPEG_GREY / JPEG_RGB)."""
    n = int(lib().sc2_jpeg_max_bytes(int(mode), int(H), int(W)))
    if n < 0:
        raise Sc2Error('jpeg_max_bytes: mode {} at {}x{} (sides 1..{})'.format(mode, H, W, JPEG_MAX_SIDE))
    return n


def jpeg_tensor_codec(x, quality, want_bytes=False, tag=None):
    """What the reference's `PILTensorModule(format='JPEG', quality=quality)` computes for every sample of x [B,C,H,W] (f32, H and W
    at most 64), in ONE launch (include/sc2_bottleneck.h: sc2_jpeg_tensor_codec): n = C // 3 + C % 3 images per sample.
    -> JpegCodecResult: recon f32 [B,C,H,W]; sizes, status: int32 [B*n] (views of `meta` [2, B*n]: one device-to-host read brings
    both), sizes = bytes of the complete file (header + segment + EOI); extrema f32 [B*n,2] (low, high); bytes uint8 [B*n, slot_bytes]
    holding each image's entropy-coded segment (size - JPEG_HEADER_BYTES[mode] - 2 bytes of it), or None.
    An image whose status is not 0 (JPEG_* bits) has size 0 and an unwritten reconstruction: the caller's host path takes that sample."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise Sc2Error('jpeg_tensor_codec: x must be a tensor on a HIP device (got {}); there is no CPU fallback in this package'
                       .format('device=' + str(x.device) if isinstance(x, torch.Tensor) else type(x)))
    if x.dtype != torch.float32:
        raise Sc2Error('jpeg_tensor_codec: an f32 tensor is required, got {}'.format(x.dtype))
    if x.dim() != 4 or x.numel() == 0:
        raise Sc2Error('jpeg_tensor_codec: a non-empty [B,C,H,W] tensor is required, got shape {}'.format(tuple(x.shape)))
    B, C, H, W = (int(v) for v in x.shape)
    if H > JPEG_MAX_SIDE or W > JPEG_MAX_SIDE:
        raise Sc2Error('jpeg_tensor_codec: {}x{} feature maps (at most {} per side)'.format(H, W, JPEG_MAX_SIDE))
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise Sc2Error('jpeg_tensor_codec: quality {!r} (an integer in 1..100)'.format(quality))
    x = x.detach().contiguous()
    n_img = B * (C // 3 + C % 3)
    recon = torch.empty_like(x)
    meta = torch.empty((2, n_img), dtype=torch.int32, device=x.device)
    extrema = torch.empty((n_img, 2), dtype=torch.float32, device=x.device)
    slot, coded = 0, None
    if want_bytes:
        slot = jpeg_max_bytes(JPEG_RGB if C >= 3 else JPEG_GREY, H, W)
        coded = torch.empty((n_img, slot), dtype=torch.uint8, device=x.device)
    with _timed(tag or 'jpeg_tensor_codec'):
        _check(lib().sc2_jpeg_tensor_codec(_ptr(x), B, C, H, W, quality, _ptr(recon), _ptr(meta[0]), _ptr(extrema), _ptr(meta[1]),
                                           _ptr(coded), slot, _stream()), 'jpeg_tensor_codec')
    return JpegCodecResult(recon, meta[0], meta[1], extrema, meta, coded, slot)


# --------------------------------------------------------------------------------------------- #
# codec input compression: 8-bit images through baseline JPEG at full image size (csrc/jpeg_image.hip)
# --------------------------------------------------------------------------------------------- #
JpegImageResult = collections.namedtuple('JpegImageResult', ['recon', 'sizes', 'bytes', 'slot_bytes'])
_jpeg_image_ws = dict()        # (device index, stream, bytes) -> the coefficient workspace of sc2_jpeg_image_codec
_JPEG_IMAGE_WS_KEPT = 4


def jpeg_image_max_bytes(C, H, W):
    """Upper bound of one image's entropy-coded segment (C: 1 grey, 3 RGB)."""
    n = int(lib().sc2_jpeg_image_max_bytes(int(C), int(H), int(W)))
    if n < 0:
        raise Sc2Error('jpeg_image_max_bytes: {} channels at {}x{} (1 or 3 channels, sides 1..{})'.format(C, H, W, JPEG_IMAGE_MAX_SIDE))
    return n


def _jpeg_image_workspace(device, n_bytes):
    """One workspace per (device, stream, size); the few most recent sizes are kept (`_stream_workspace`)."""
    return _stream_workspace(_jpeg_image_ws, _JPEG_IMAGE_WS_KEPT, device, n_bytes)


def jpeg_image_codec(x_u8, quality, want_bytes=False, tag=None):
    """What the reference's `PILImageModule(format='JPEG', quality=quality)` computes for every image of x_u8 [B,C,H,W] (uint8 on the
    device, C 3: RGB, 1: grey; any non-negative strides: the permuted view of an HWC stack is read in place; sides up to
    JPEG_IMAGE_MAX_SIDE), in three launches (include/sc2_bottleneck.h: sc2_jpeg_image_codec).
    -> JpegImageResult: recon uint8 [B,C,H,W] contiguous, the decoded pixels; sizes int32 [B], bytes of the complete file (header +
    segment + EOI); bytes uint8 [B, slot_bytes] holding each image's entropy-coded segment (size - JPEG_HEADER_BYTES[mode] - 2 bytes
    of it), or None."""
    if not isinstance(x_u8, torch.Tensor) or not x_u8.is_cuda:
        raise Sc2Error('jpeg_image_codec: x must be a tensor on a HIP device (got {}); there is no CPU fallback in this package'
                       .format('device=' + str(x_u8.device) if isinstance(x_u8, torch.Tensor) else type(x_u8)))
    if x_u8.dtype != torch.uint8:
        raise Sc2Error('jpeg_image_codec: a uint8 tensor is required, got {}'.format(x_u8.dtype))
    if x_u8.dim() != 4 or x_u8.numel() == 0:
        raise Sc2Error('jpeg_image_codec: a non-empty [B,C,H,W] tensor is required, got shape {}'.format(tuple(x_u8.shape)))
    B, C, H, W = (int(v) for v in x_u8.shape)
    if C not in (1, 3):
        raise Sc2Error('jpeg_image_codec: {} channels (1: grey, 3: RGB)'.format(C))
    if H > JPEG_IMAGE_MAX_SIDE or W > JPEG_IMAGE_MAX_SIDE:
        raise Sc2Error('jpeg_image_codec: {}x{} images (at most {} per side)'.format(H, W, JPEG_IMAGE_MAX_SIDE))
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise Sc2Error('jpeg_image_codec: quality {!r} (an integer in 1..100)'.format(quality))
    x_u8 = x_u8.detach()
    sb, sc, sh, sw = (int(v) for v in x_u8.stride())
    dev = x_u8.device
    recon = torch.empty((B, C, H, W), dtype=torch.uint8, device=dev)
    sizes = torch.empty((B,), dtype=torch.int32, device=dev)
    slot, coded = 0, None
    if want_bytes:
        slot = jpeg_image_max_bytes(C, H, W)
        coded = torch.empty((B, slot), dtype=torch.uint8, device=dev)
    ws_bytes = int(lib().sc2_jpeg_image_workspace_bytes(B, C, H, W))
    ws = _jpeg_image_workspace(dev, ws_bytes)
    with _timed(tag or 'jpeg_image_codec'):
        _check(lib().sc2_jpeg_image_codec(_ptr(x_u8), sb, sc, sh, sw, B, C, H, W, quality, _ptr(recon), _ptr(sizes), _ptr(coded), slot,
                                          _ptr(ws), ws_bytes, _stream()), 'jpeg_image_codec')
    return JpegImageResult(recon, sizes, coded, slot)


# --------------------------------------------------------------------------------------------- #
# the detection transform around the image codec (csrc/rcnn_input.hip)
# --------------------------------------------------------------------------------------------- #
def rcnn_resize_u8(image, oh, ow, out=None, status=None, tag=None):
    """f32 image [C,H,W] on the device (C 1 or 3, any non-negative strides, values in [0, 1]) -> (uint8 [C,oh,ow], status int32 [1]):
    `F.interpolate(image[None], ..., mode='bilinear', align_corners=False)[0].mul(255).byte()` at the size (oh, ow) in one launch
    (include/sc2_bottleneck.h: sc2_rcnn_resize_u8).  status is non-zero when the kernel read a NaN or a value outside [0, 1]: the
    bytes are then unspecified.  `out`: a contiguous uint8 [C,oh,ow] tensor to write; `status`: an int32 tensor of one element the
    caller has CLEARED (e.g. one element of a zeroed vector that is read back once for many images)."""
    _dev(image, 'rcnn_resize_u8: image')
    if image.dtype != torch.float32 or image.dim() != 3:
        raise Sc2Error('rcnn_resize_u8: a float32 [C,H,W] tensor is required, got {} {}'.format(image.dtype, tuple(image.shape)))
    C, H, W = (int(v) for v in image.shape)
    oh, ow = int(oh), int(ow)
    if C not in (1, 3):
        raise Sc2Error('rcnn_resize_u8: {} channels (1 or 3)'.format(C))
    if not (1 <= min(H, W, oh, ow) and max(H, W, oh, ow) <= JPEG_IMAGE_MAX_SIDE):
        raise Sc2Error('rcnn_resize_u8: {}x{} -> {}x{} (sides 1..{})'.format(H, W, oh, ow, JPEG_IMAGE_MAX_SIDE))
    image = image.detach()
    dev = image.device
    if out is None:
        out = torch.empty((C, oh, ow), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (C, oh, ow) or not out.is_contiguous() or out.device != dev:
        raise ValueError('rcnn_resize_u8: out must be a contiguous uint8 tensor of shape {} on {}'.format((C, oh, ow), dev))
    if status is None:
        status = torch.zeros((1,), dtype=torch.int32, device=dev)
    elif status.dtype != torch.int32 or status.numel() != 1 or status.device != dev:
        raise ValueError('rcnn_resize_u8: status must be an int32 tensor of one element on {}'.format(dev))
    sc, sh, sw = (int(v) for v in image.stride())
    with _timed(tag or 'rcnn_resize_u8'):
        _check(lib().sc2_rcnn_resize_u8(_ptr(image), sc, sh, sw, C, H, W, _ptr(out), oh, ow, _ptr(status), _stream()), 'rcnn_resize_u8')
    return out, status


def rcnn_normalize_pad(pixels_u8, mean, std, out_slot, tag=None):
    """uint8 pixels [C,h,w] on the device (contiguous: the codec's recon) -> out_slot f32 [C,Hp,Wp] (contiguous, Hp >= h, Wp >= w: one
    image's slot of the batch tensor): `(to_tensor(pixels) - mean) / std` inside the image, +0.0 outside, every element of the slot
    written, in one launch (include/sc2_bottleneck.h: sc2_rcnn_normalize_pad).  mean, std: C numbers.  -> out_slot."""
    _dev(pixels_u8, 'rcnn_normalize_pad: pixels')
    _dev(out_slot, 'rcnn_normalize_pad: out_slot')
    if pixels_u8.dtype != torch.uint8 or pixels_u8.dim() != 3 or not pixels_u8.is_contiguous():
        raise Sc2Error('rcnn_normalize_pad: a contiguous uint8 [C,h,w] tensor is required, got {} {}'.format(pixels_u8.dtype, tuple(pixels_u8.shape)))
    C, h, w = (int(v) for v in pixels_u8.shape)
    if out_slot.dtype != torch.float32 or out_slot.dim() != 3 or out_slot.shape[0] != C or not out_slot.is_contiguous() or \
            out_slot.device != pixels_u8.device:
        raise Sc2Error('rcnn_normalize_pad: out_slot must be a contiguous float32 [{},Hp,Wp] tensor on {}, got {} {}'.format(
            C, pixels_u8.device, out_slot.dtype, tuple(out_slot.shape)))
    mean, std = [float(v) for v in mean], [float(v) for v in std]
    if len(mean) != C or len(std) != C:
        raise ValueError('rcnn_normalize_pad: {} mean and {} std values for {} channels'.format(len(mean), len(std), C))
    Hp, Wp = int(out_slot.shape[1]), int(out_slot.shape[2])
    fm, fs = (ctypes.c_float * C)(*mean), (ctypes.c_float * C)(*std)
    with _timed(tag or 'rcnn_normalize_pad'):
        _check(lib().sc2_rcnn_normalize_pad(_ptr(pixels_u8), C, h, w, fm, fs, _ptr(out_slot.detach()), Hp, Wp, _stream()), 'rcnn_normalize_pad')
    return out_slot


class _InputCall(object):
    """What det_input, seg_augment and cls_input repeat around their call: the flat uint8 source buffer on the device, mean / std as
    two `c_float * 3`, and an output tensor (the caller's, checked; or a new one)."""
    def __init__(self, who, buf):
        _dev(buf, who + ': buf')
        if buf.dtype != torch.uint8 or buf.dim() != 1 or not buf.is_contiguous():
            raise Sc2Error('{}: a flat contiguous uint8 buffer is required, got {} {}'.format(who, buf.dtype, tuple(buf.shape)))
        self.who, self.buf, self.nbytes, self.dev = who, buf, int(buf.numel()), buf.device

    def norm(self, mean, std, error, non_zero):
        """-> (mean, std) as `c_float * 3`; `error` is what anything else raises; non_zero: a zero std is refused here, too"""
        mean, std = [float(v) for v in mean], [float(v) for v in std]
        if len(mean) != 3 or len(std) != 3 or (non_zero and any(v == 0.0 for v in std)):
            raise error('{}: three mean and three {}std values are required'.format(self.who, 'non-zero ' if non_zero else ''))
        return (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)

    def out(self, t, name, dtype, shape):
        """t (None: a new one) as the contiguous tensor of that dtype and shape on the buffer's device; a name in `shape`: any size"""
        if t is None:
            return torch.empty(shape, dtype=dtype, device=self.dev)
        _dev(t, '{}: {}'.format(self.who, name))
        fits = t.dim() == len(shape) and all(isinstance(want, str) or int(have) == want for have, want in zip(t.shape, shape))
        if t.dtype != dtype or not fits or not t.is_contiguous() or t.device != self.dev:
            raise Sc2Error('{}: {} must be a contiguous {} [{}] tensor on {}, got {} {}'.format(
                self.who, name, str(dtype).split('.')[-1], ','.join(str(v) for v in shape), self.dev, t.dtype, tuple(t.shape)))
        return t


class _DescTable(collections.namedtuple('_DescTable', ['who', 'fields', 'defaults', 'width', 'max_batch'])):
    """The descriptor table of an input kernel as its `*_desc` / `*_check` pair declares it: `who` for the messages, the names of a row's
    leading words, `defaults` (the fields given -> (name, value) of those that may be left out), a row's int32 words, the most rows."""
    def row(self, fields):
        for name, value in self.defaults(fields):
            fields.setdefault(name, value)
        row = np.zeros(self.width, dtype=np.int32)
        row[:len(self.fields)] = [int(fields.pop(name)) for name in self.fields]
        assert not fields, '{}_desc: unknown fields {}'.format(self.who, sorted(fields))
        return row

    def rows(self, desc, nbytes, oh, ow):
        """The front of a check: the table's shape, the output slot and the buffer's size; then a `_DescRow` per row for the rules."""
        desc = np.asarray(desc)
        if desc.ndim != 2 or desc.shape[1] != self.width or desc.shape[0] < 1 or desc.shape[0] > self.max_batch:
            raise ValueError('{}: a descriptor table [1..{}, {}] is required, got {}'.format(self.who, self.max_batch, self.width, desc.shape))
        if not (1 <= oh <= SEG_AUGMENT_MAX_SIDE and 1 <= ow <= SEG_AUGMENT_MAX_SIDE):
            raise ValueError('{}: a {} x {} output slot (sides 1..{})'.format(self.who, oh, ow, SEG_AUGMENT_MAX_SIDE))
        if not 1 <= nbytes <= 0x7FFFFFFF:
            raise ValueError('{}: a source buffer of {} bytes (1..2^31-1)'.format(self.who, nbytes))
        return [_DescRow(self.who, i, dict(zip(self.fields, row)), nbytes) for i, row in enumerate(desc.tolist())]


class _DescRow(collections.namedtuple('_DescRow', ['who', 'i', 'f', 'nbytes'])):
    """Row i of a `_DescTable` under check: `f`, its fields by name, and the rules the tables share"""
    def refuse(self, name, why):
        raise ValueError('{}: sample {}: {} = {}: {}'.format(self.who, self.i, name, self.f[name], why))

    def sides(self, *names):
        for name in names:
            if not 1 <= self.f[name] <= SEG_AUGMENT_MAX_SIDE:
                self.refuse(name, 'sides are 1..{}'.format(SEG_AUGMENT_MAX_SIDE))

    def inside(self, name, k, what):      # the k * h * w bytes at offset `name`
        if self.f[name] < 0 or self.f[name] + k * self.f['h'] * self.f['w'] > self.nbytes:
            self.refuse(name, 'the {} lies outside the buffer of {} bytes'.format(what, self.nbytes))

    def flip(self):
        if self.f['flip'] not in (0, 1):
            self.refuse('flip', '0 or 1')


def det_input(buf, rows, mean, std, out, tag=None):
    """The detector's input transform of a planned batch (include/sc2_bottleneck.h: sc2_det_input).  buf: flat contiguous uint8 device
    tensor holding the interleaved [h,w,3] sources; rows: integers [n, DET_INPUT_ROW_INTS] on the host -- (byte offset, h, w, oh, ow,
    flip) per sample, checked by the library on the host before anything is launched (a bad row raises Sc2Error and `out` is
    untouched); mean, std: three numbers each; out: a contiguous float32 [n,3,Hp,Wp] device tensor, every element of which is written
    (+0.0 outside a sample's (oh, ow)).  One launch per DET_INPUT_MAX_BATCH samples.  -> out."""
    call = _InputCall('det_input', buf)
    table = np.ascontiguousarray(np.asarray(rows.numpy() if isinstance(rows, torch.Tensor) else rows, dtype=np.int64))
    if table.ndim != 2 or table.shape[0] < 1 or table.shape[1] != DET_INPUT_ROW_INTS:
        raise Sc2Error('det_input: a descriptor table [n >= 1, {}] is required, got {}'.format(DET_INPUT_ROW_INTS, table.shape))
    if np.abs(table).max() > 0x7FFFFFFF:
        raise Sc2Error('det_input: a descriptor field beyond int32')
    table = table.astype(np.int32)
    n = int(table.shape[0])
    dst = call.out(out, 'out', torch.float32, (n, 3, 'Hp', 'Wp')).detach()
    fm, fs = call.norm(mean, std, Sc2Error, non_zero=False)      # (a zero std is the library's to refuse)
    Hp, Wp = int(out.shape[2]), int(out.shape[3])
    with _timed(tag or 'det_input'):
        for i0 in range(0, n, DET_INPUT_MAX_BATCH):
            part = np.ascontiguousarray(table[i0:i0 + DET_INPUT_MAX_BATCH])
            rc = lib().sc2_det_input(_ptr(buf), call.nbytes, ctypes.c_void_p(part.ctypes.data), int(part.shape[0]), fm, fs,
                                     _ptr(dst[i0:i0 + DET_INPUT_MAX_BATCH]), Hp, Wp, _stream())
            if rc != 0:
                raise Sc2Error('det_input failed (code {}): {}'.format(rc, last_error()))
    return out


# --------------------------------------------------------------------------------------------- #
# segmentation training input: the PASCAL augmentation chain of a batch from its source bytes (csrc/seg_augment.hip)
# --------------------------------------------------------------------------------------------- #
SEG_AUGMENT_FIELDS = ('image_offset', 'mask_offset', 'h', 'w', 'nh', 'nw', 'flip', 'top', 'left', 'ext_h', 'ext_w', 'pad_h', 'pad_w')
SegAugment = collections.namedtuple('SegAugment', ['images', 'targets', 'status', 'workspace'])
_SEG_AUGMENT_TABLE = _DescTable('seg_augment', SEG_AUGMENT_FIELDS, lambda f: (
    ('pad_h', max(f['nh'], f['top'] + f['ext_h'])), ('pad_w', max(f['nw'], f['left'] + f['ext_w']))), SEG_AUGMENT_DESC_INTS, SEG_AUGMENT_MAX_BATCH)


def seg_augment_desc(**fields):
    """One descriptor row (int32 [SEG_AUGMENT_DESC_INTS]) from SEG_AUGMENT_FIELDS by name; pad_h / pad_w (the padded size, which only
    `seg_augment_check` reads) default to max(nh, top + ext_h) / max(nw, left + ext_w)."""
    return _SEG_AUGMENT_TABLE.row(fields)


def seg_augment_check(desc, nbytes, oh, ow):
    """Refuses a malformed descriptor table on the host, before any launch (ValueError naming the sample and the field): sides below
    1 or above SEG_AUGMENT_MAX_SIDE, offsets outside the buffer, a flip that is not 0 / 1, an extent outside its slot, a padded size
    smaller than the resized one, a window outside the padded image.  desc: integer array [n, SEG_AUGMENT_DESC_INTS]."""
    for r in _SEG_AUGMENT_TABLE.rows(desc, nbytes, oh, ow):
        f = r.f
        r.sides('h', 'w', 'nh', 'nw')
        r.inside('image_offset', 3, 'image')
        r.inside('mask_offset', 1, 'mask')
        r.flip()
        for name, limit in (('ext_h', oh), ('ext_w', ow)):
            if not 1 <= f[name] <= limit:
                r.refuse(name, 'the extent is 1..{}'.format(limit))
        for name, resized in (('pad_h', 'nh'), ('pad_w', 'nw')):
            if f[name] < f[resized] or f[name] > SEG_AUGMENT_MAX_SIDE:
                r.refuse(name, 'the padded size is {}..{}'.format(f[resized], SEG_AUGMENT_MAX_SIDE))
        for name, ext, padded in (('top', 'ext_h', 'pad_h'), ('left', 'ext_w', 'pad_w')):
            if f[name] < 0 or f[name] + f[ext] > f[padded]:
                r.refuse(name, 'the window of {} lies outside the padded image of {}'.format(f[ext], f[padded]))
    return np.asarray(desc)


def seg_augment(buf, desc, size, mean, std, images_out=None, targets_out=None, return_workspace=False, tag=None):
    """The augmentation chain of a batch on the device (include/sc2_bottleneck.h: sc2_seg_augment).  buf: uint8 device tensor holding the
    sources and masks; desc: integer array / CPU tensor [n, SEG_AUGMENT_DESC_INTS] (rows from `seg_augment_desc`), checked by
    `seg_augment_check` before anything is launched; size: (oh, ow); mean, std: three numbers each.  images_out f32 [n,3,oh,ow] /
    targets_out int64 [n,oh,ow]: a caller's contiguous tensors to write into.
    -> SegAugment(images, targets, status int32 [n] on the device, workspace): nothing is read back; a sample whose status is not 0
    (SEG_AUGMENT_RATIO: an axis shrinks by more than 4) has unspecified outputs.  `workspace` (tests) is the int32 table
    [n, ow + oh, SEG_AUGMENT_ENTRY_INTS] when asked for, else None."""
    call = _InputCall('seg_augment', buf)
    oh, ow = int(size[0]), int(size[1])
    table = np.ascontiguousarray(desc.numpy() if isinstance(desc, torch.Tensor) else desc)
    seg_augment_check(table, call.nbytes, oh, ow)
    n, dev = int(table.shape[0]), call.dev
    fm, fs = call.norm(mean, std, ValueError, non_zero=True)
    d_desc = torch.from_numpy(table.astype(np.int32)).to(dev, non_blocking=True)
    images = call.out(images_out, 'images_out', torch.float32, (n, 3, oh, ow))
    targets = call.out(targets_out, 'targets_out', torch.int64, (n, oh, ow))
    ws_bytes = int(lib().sc2_seg_augment_workspace(n, oh, ow))
    assert ws_bytes == n * (oh + ow) * SEG_AUGMENT_ENTRY_INTS * 4
    ws = torch.empty((n, ow + oh, SEG_AUGMENT_ENTRY_INTS), dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    with _timed(tag or 'seg_augment'):
        _check(lib().sc2_seg_augment(_ptr(buf), call.nbytes, _ptr(d_desc), n, oh, ow, fm, fs, _ptr(images), _ptr(targets), _ptr(ws),
                                     _ptr(status), _stream()), 'seg_augment')
    return SegAugment(images, targets, status, ws if return_workspace else None)


# --------------------------------------------------------------------------------------------- #
# classification input: the ImageNet train / eval chains of a batch from stored boxes of its sources (csrc/cls_input.hip)
# --------------------------------------------------------------------------------------------- #
CLS_INPUT_FIELDS = ('offset', 'h', 'w', 'full_h', 'full_w', 'row0', 'col0', 'nh', 'nw', 'flip', 'top', 'left')
ClsInput = collections.namedtuple('ClsInput', ['images', 'status'])
_CLS_INPUT_TABLE = _DescTable('cls_input', CLS_INPUT_FIELDS, lambda f: (
    ('full_h', f.get('h')), ('full_w', f.get('w')), ('row0', 0), ('col0', 0), ('flip', 0), ('top', 0), ('left', 0)), CLS_INPUT_DESC_INTS,
                              CLS_INPUT_MAX_BATCH)


def cls_input_desc(**fields):
    """One descriptor row (int32 [CLS_INPUT_DESC_INTS]) from CLS_INPUT_FIELDS by name.  offset, h, w, nh, nw are required; the rest
    default to the train form: full_h / full_w = h / w, row0 = col0 = 0, flip = 0, top = left = 0."""
    return _CLS_INPUT_TABLE.row(fields)


def cls_input_check(desc, nbytes, oh, ow):
    """Refuses a malformed descriptor table on the host, before any launch (ValueError naming the sample and the field): sides below 1
    or above SEG_AUGMENT_MAX_SIDE, a stored box outside the buffer or outside the full image, a flip that is not 0 / 1, a window outside
    the resized image.  A ratio above 4 and a tap outside the stored box are the kernel's to flag (its status word): they are well
    formed.  desc: integer array [n, CLS_INPUT_DESC_INTS]."""
    for r in _CLS_INPUT_TABLE.rows(desc, nbytes, oh, ow):
        f = r.f
        r.sides('h', 'w', 'full_h', 'full_w', 'nh', 'nw')
        r.inside('offset', 3, 'stored box')
        for name, side, full in (('row0', 'h', 'full_h'), ('col0', 'w', 'full_w')):
            if f[name] < 0 or f[name] + f[side] > f[full]:
                r.refuse(name, 'the stored box of {} lies outside the full image of {}'.format(f[side], f[full]))
        r.flip()
        for name, ext, resized in (('top', oh, 'nh'), ('left', ow, 'nw')):
            if f[name] < 0 or f[name] + ext > f[resized]:
                r.refuse(name, 'the window of {} lies outside the resized image of {}'.format(ext, f[resized]))
    return np.asarray(desc)


def cls_input(buf, desc, size, mean, std, images_out=None, tag=None):
    """The classification input chain of a batch on the device (include/sc2_bottleneck.h: sc2_cls_input).  buf: uint8 device tensor
    holding the stored boxes; desc: integer array / CPU tensor [n, CLS_INPUT_DESC_INTS] (rows from `cls_input_desc`), checked by
    `cls_input_check` before anything is launched; size: (oh, ow); mean, std: three numbers each.  images_out f32 [n,3,oh,ow]: a
    caller's contiguous tensor to write into.
    -> ClsInput(images, status int32 [n] on the device): nothing is read back; a sample whose status is not 0 (CLS_INPUT_RATIO: an
    axis shrinks by more than 4; CLS_INPUT_TAP: a tap outside its stored box) has its slot unwritten."""
    call = _InputCall('cls_input', buf)
    oh, ow = int(size[0]), int(size[1])
    table = np.ascontiguousarray(desc.numpy() if isinstance(desc, torch.Tensor) else desc)
    cls_input_check(table, call.nbytes, oh, ow)
    n, dev = int(table.shape[0]), call.dev
    fm, fs = call.norm(mean, std, ValueError, non_zero=True)
    d_desc = torch.from_numpy(table.astype(np.int32)).to(dev, non_blocking=True)
    images = call.out(images_out, 'images_out', torch.float32, (n, 3, oh, ow))
    assert int(lib().sc2_cls_input_workspace(n, oh, ow)) == 0      # one launch, tables in LDS: nothing to allocate
    status = torch.empty(n, dtype=torch.int32, device=dev)
    with _timed(tag or 'cls_input'):
        _check(lib().sc2_cls_input(_ptr(buf), call.nbytes, _ptr(d_desc), n, oh, ow, fm, fs, _ptr(images), _ptr(status), _stream()), 'cls_input')
    return ClsInput(images, status)


# --------------------------------------------------------------------------------------------- #
# COCO box AP: matching of every (image, category) segment and the precision / recall curves (csrc/coco.hip)
# --------------------------------------------------------------------------------------------- #
def _coco_arg(t, name, dtype, shape):
    _dev(t, name)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError('{}: expected a contiguous {} tensor of shape {}, got {} {}{}'.format(
            name, dtype, tuple(shape), t.dtype, tuple(t.shape), '' if t.is_contiguous() else ' (not contiguous)'))
    return t


def coco_match(dets, gts, gt_area, gt_crowd, det_off, gt_off, iou_thrs, area_rng, flags=None, npig=None, tag=None):
    """COCOeval's matching of every (image, category) segment in ONE launch (include/sc2_bottleneck.h: sc2_coco_match).
    dets: f64 [n_det,4] xywh in processing order within each segment; gts: f64 [n_gt,4] xywh, gt_area: f64 [n_gt], gt_crowd: u8 [n_gt];
    det_off / gt_off: i32 [n_seg+1]; iou_thrs: f64 [10]; area_rng: f64 [4,2] -> (flags i32 [n_det,4]: bit t matched, bit 10+t ignored;
    npig i32 [n_seg,4]), on the device; nothing synchronises.  `flags` / `npig`: a caller's buffers to write into."""
    n_det, n_gt = int(dets.shape[0]), int(gts.shape[0])
    n_seg = int(det_off.shape[0]) - 1
    if n_seg < 0 or gt_off.shape[0] != n_seg + 1:
        raise ValueError('coco_match: {} detection offsets and {} ground-truth offsets (n_seg + 1 of each)'.format(det_off.shape[0], gt_off.shape[0]))
    dev = _coco_arg(dets, 'dets', torch.float64, (n_det, 4)).device
    _coco_arg(gts, 'gts', torch.float64, (n_gt, 4))
    _coco_arg(gt_area, 'gt_area', torch.float64, (n_gt,))
    _coco_arg(gt_crowd, 'gt_crowd', torch.uint8, (n_gt,))
    _coco_arg(det_off, 'det_off', torch.int32, (n_seg + 1,))
    _coco_arg(gt_off, 'gt_off', torch.int32, (n_seg + 1,))
    _coco_arg(iou_thrs, 'iou_thrs', torch.float64, (COCO_THRS,))
    _coco_arg(area_rng, 'area_rng', torch.float64, (COCO_AREAS, 2))
    if flags is None:
        flags = torch.empty((n_det, COCO_AREAS), dtype=torch.int32, device=dev)
    if npig is None:
        npig = torch.empty((n_seg, COCO_AREAS), dtype=torch.int32, device=dev)
    _coco_arg(flags, 'flags', torch.int32, (n_det, COCO_AREAS))
    _coco_arg(npig, 'npig', torch.int32, (n_seg, COCO_AREAS))
    for t in (gts, gt_area, gt_crowd, det_off, gt_off, iou_thrs, area_rng, flags, npig):
        if t.device != dev:
            raise ValueError('coco_match: tensors on {} and {}'.format(dev, t.device))
    if n_seg == 0:
        return flags, npig
    ws = torch.empty(int(lib().sc2_coco_match_ws_bytes(n_gt)), dtype=torch.uint8, device=dev)
    with _timed(tag or 'coco_match'):
        _check(lib().sc2_coco_match(_ptr(dets), _ptr(gts), _ptr(gt_area), _ptr(gt_crowd), _ptr(det_off), _ptr(gt_off), n_seg, n_det, n_gt,
                                    _ptr(iou_thrs), _ptr(area_rng), _ptr(flags), _ptr(npig), _ptr(ws), _stream()), 'coco_match')
    return flags, npig


def coco_accumulate(order, cat_off, flags, rank, npig, rec_thrs, max_dets, tag=None):
    """COCOeval's accumulate for every (category, area range, maxDet) in ONE launch (include/sc2_bottleneck.h: sc2_coco_accumulate).
    order: i32 [n_order], category k's detections in its score-sorted order at cat_off[k] .. cat_off[k+1]-1 (indices into flags / rank);
    cat_off: i32 [K+1]; flags: i32 [n_det,4] of coco_match; rank: i32 [n_det]; npig: i32 [K,4] category totals; rec_thrs: f64 [101];
    max_dets: i32 [3] -> (precision f64 [10,101,K,4,3], recall f64 [10,K,4,3]) on the device; nothing synchronises."""
    n_order, n_det, K = int(order.shape[0]), int(flags.shape[0]), int(cat_off.shape[0]) - 1
    if K < 0:
        raise ValueError('coco_accumulate: cat_off is empty (K + 1 offsets)')
    dev = _coco_arg(order, 'order', torch.int32, (n_order,)).device
    _coco_arg(cat_off, 'cat_off', torch.int32, (K + 1,))
    _coco_arg(flags, 'flags', torch.int32, (n_det, COCO_AREAS))
    _coco_arg(rank, 'rank', torch.int32, (n_det,))
    _coco_arg(npig, 'npig', torch.int32, (K, COCO_AREAS))
    _coco_arg(rec_thrs, 'rec_thrs', torch.float64, (COCO_RECS,))
    _coco_arg(max_dets, 'max_dets', torch.int32, (COCO_MAXDETS,))
    for t in (cat_off, flags, rank, npig, rec_thrs, max_dets):
        if t.device != dev:
            raise ValueError('coco_accumulate: tensors on {} and {}'.format(dev, t.device))
    precision = torch.empty((COCO_THRS, COCO_RECS, K, COCO_AREAS, COCO_MAXDETS), dtype=torch.float64, device=dev)
    recall = torch.empty((COCO_THRS, K, COCO_AREAS, COCO_MAXDETS), dtype=torch.float64, device=dev)
    with _timed(tag or 'coco_accumulate'):
        _check(lib().sc2_coco_accumulate(_ptr(order), _ptr(cat_off), _ptr(flags), _ptr(rank), _ptr(npig), _ptr(rec_thrs), _ptr(max_dets), K,
                                         n_order, n_det, _ptr(precision), _ptr(recall), _stream()), 'coco_accumulate')
    return precision, recall


def bn_train_fwd(x_nhwc, gamma, beta, running_mean, running_var, momentum, eps, relu, residual=None, tag=None):
    """BatchNorm2d with batch statistics on a bf16 NHWC map (+ residual, ReLU): -> (y, save_mean, save_rstd).  gamma / beta /
    running_* : f32 [C] (running_* may be None); running statistics are updated in place as nn.BatchNorm2d does."""
    _dev(x_nhwc, 'x')
    assert x_nhwc.dtype == torch.bfloat16 and x_nhwc.dim() == 4 and x_nhwc.is_contiguous()
    C = x_nhwc.shape[3]
    M = x_nhwc.numel() // C
    if M <= 1:
        raise ValueError('Expected more than 1 value per channel when training, got input size {}'.format(tuple(x_nhwc.shape)))
    for t in (gamma, beta, running_mean, running_var):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == C and t.device == x_nhwc.device)
    assert residual is None or (residual.dtype == torch.bfloat16 and residual.shape == x_nhwc.shape and residual.is_contiguous())
    y = torch.empty_like(x_nhwc)
    stats = torch.empty((2, C), dtype=torch.float32, device=x_nhwc.device)      # save_mean, save_rstd
    ws = torch.empty((int(lib().sc2_bn_ws_floats(M, C)),), dtype=torch.float32, device=x_nhwc.device)
    with _timed(tag or 'bn.fwd'):
        _check(lib().sc2_bn_train_fwd(_ptr(x_nhwc), _ptr(residual), _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var),
                                      float(momentum), float(eps), 1 if relu else 0, _ptr(y), stats[0].data_ptr(), stats[1].data_ptr(),
                                      _ptr(ws), M, C, _stream()), 'bn_train_fwd')
    return y, stats[0], stats[1]


def bn_train_bwd(dy, x_nhwc, y_or_none, gamma, save_mean, save_rstd, want_dz=False, tag=None):
    """-> (dx bf16, dz bf16 or None, dgamma f32 [C], dbeta f32 [C]); y_or_none: the forward's output if it applied the ReLU."""
    _dev(dy, 'dy')
    assert dy.dtype == torch.bfloat16 and dy.is_contiguous() and dy.shape == x_nhwc.shape and x_nhwc.is_contiguous()
    assert y_or_none is None or (y_or_none.is_contiguous() and y_or_none.shape == x_nhwc.shape)
    C = x_nhwc.shape[3]
    M = x_nhwc.numel() // C
    dx = torch.empty_like(x_nhwc)
    dz = torch.empty_like(x_nhwc) if want_dz else None
    out = torch.empty((2, C), dtype=torch.float32, device=dy.device)           # dgamma, dbeta
    ws = torch.empty((int(lib().sc2_bn_ws_floats(M, C)),), dtype=torch.float32, device=dy.device)
    with _timed(tag or 'bn.bwd'):
        _check(lib().sc2_bn_train_bwd(_ptr(dy), _ptr(x_nhwc), _ptr(y_or_none), _ptr(gamma), _ptr(save_mean), _ptr(save_rstd), _ptr(dx),
                                      _ptr(dz), out[0].data_ptr(), out[1].data_ptr(), _ptr(ws), M, C, _stream()), 'bn_train_bwd')
    return dx, dz, out[0], out[1]


def fc_fwd(a, w_frag, bias, tag=None):
    """out f32 [M, Npad] = a [M, K] (bf16) @ W^T + bias; w_frag = pack_weight_fragments(W [Npad, K]), Npad % 16 == 0."""
    for t, name in ((a, 'a'), (w_frag, 'w_frag'), (bias, 'bias')):
        _dev(t, name)
    assert a.dtype == torch.bfloat16 and a.dim() == 2 and a.is_contiguous()
    M, K = a.shape
    npad = w_frag.shape[0] * 16
    assert w_frag.dtype == torch.bfloat16 and w_frag.is_contiguous() and tuple(w_frag.shape) == (npad // 16, K // 32, 64, 8)
    assert bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == npad
    out = torch.empty((M, npad), dtype=torch.float32, device=a.device)
    with _timed(tag or 'fc'):
        _check(lib().sc2_fc_fwd(_ptr(a), _ptr(w_frag), _ptr(bias), _ptr(out), M, K, npad, _stream()), 'fc_fwd')
    return out


def pack_weight_fragments(w2d):
    """[N, K] matrix (row = output channel) -> bf16 MFMA-fragment blocks [N/16][K/32][64][8]: entry (jt, ks, lane =
    fq*16 + frow, e) = w2d[jt*16 + frow, ks*32 + fq*8 + e], one operand fragment = 1 KB contiguous."""
    _dev(w2d, 'w2d')
    n, k = w2d.shape
    assert n % 16 == 0 and k % 32 == 0
    g = w2d.detach().to(torch.bfloat16).reshape(n // 16, 16, k // 32, 4, 8)      # jt, frow, ks, fq, e
    return g.permute(0, 2, 3, 1, 4).contiguous().reshape(n // 16, k // 32, 64, 8)


def conv1x1_kres_supported(cin, cout, kh, kw, stride, pad):
    """True if this 1x1 conv runs on the weights-in-registers kernel (K = 1024 or 2048, stride 1 or 2)."""
    (sh, sw), (ph, pw) = _pair2(stride), _pair2(pad)
    mode = str(host_policy.conv_kres)          # A/B switch (tools/): 0 off, 2 = also the K = 2048 layers
    if mode == '0':
        return False
    if cin == 2048 and mode != '2':   # measured: layer4 conv1 (2048 -> 512, 12 544 pixels) 0.065 ms vs 0.063 ms on the tile kernel
        return False
    return (kh, kw, ph, pw) == (1, 1, 0, 0) and sh == sw and bool(lib().sc2_conv1x1_kres_supported(cin, cout, sh))


# the two weight streams of these kernels: (the dimension that counts 16-channel tiles of Cout, the shape as a function of (Cin, Cout))
_ROWS_FRAG = (0, lambda cin, cout: (cout // 16, cin // 32, 64, 8))                      # pack_weight_fragments(w[Cout, Cin])
_WIN_FRAG = {taps: (1, lambda cin, cout, taps=taps: (cin // 32 * taps, cout // 16, 64, 8)) for taps in (1, 9)}   # pack_conv_win, by KH * KW


def _frag_conv_fwd(what, x_nhwc, w_frag, bias, frag_shape, stride, relu, tag, *extra, stride_arg=True, out=None):
    """The frame of the (x, w_frag, bias) -> bf16 NHWC wrappers around `sc2_<what>(x, w_frag, bias, *extra, out, N, H, W, Cin, Cout,
    [stride,] relu, stream)`.  Checks x, the fragment stream (`frag_shape`: one of the two rules above) and the bias; makes the output
    [N, (H - 1) // stride + 1, (W - 1) // stride + 1, Cout] -- a 1x1 conv without padding or a 3x3 conv with padding 1 -- or views `out`,
    a contiguous bf16 tensor of that size, as it; checks each of `extra`, (name, tensor or None) operands laid out like the output
    ('mask' excludes relu); launches under the kernel timer (default tag: `what` without '_fwd')."""
    for t, name in ((x_nhwc, 'x'), (w_frag, 'w_frag'), (bias, 'bias')):
        _dev(t, name)
    assert x_nhwc.dtype == torch.bfloat16 and x_nhwc.dim() == 4 and x_nhwc.is_contiguous()
    N, H, W, Cin = x_nhwc.shape
    cout = w_frag.shape[frag_shape[0]] * 16
    assert w_frag.dtype == torch.bfloat16 and w_frag.is_contiguous() and tuple(w_frag.shape) == frag_shape[1](Cin, cout)
    assert bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == cout
    shape = (N, (H - 1) // stride + 1, (W - 1) // stride + 1, cout)
    if out is None:
        out = torch.empty(shape, dtype=torch.bfloat16, device=x_nhwc.device)
    else:
        _dev(out, 'out')
        assert out.dtype == torch.bfloat16 and out.is_contiguous() and out.numel() == N * shape[1] * shape[2] * cout
        out = out.view(shape)
    ptrs = [_ptr(x_nhwc), _ptr(w_frag), _ptr(bias)]
    for name, t in extra:
        if t is not None:
            _dev(t, name)
            assert t.dtype == torch.bfloat16 and t.is_contiguous() and tuple(t.shape) == shape and not (relu and name == 'mask'), name
        ptrs.append(_ptr(t))
    dims = (N, H, W, Cin, cout, stride) if stride_arg else (N, H, W, Cin, cout)
    with _timed(tag or what[:-4]):
        _check(getattr(lib(), 'sc2_' + what)(*ptrs, _ptr(out), *dims, 1 if relu else 0, _stream()), what)
    return out


def conv1x1_kres_fwd(x_nhwc, w_frag, bias, stride=1, relu=False, tag=None):
    """x bf16 [N,H,W,Cin] -> bf16 [N,OH,OW,Cout]; w_frag = pack_weight_fragments(w[Cout, Cin]); Cin 1024 or 2048."""
    return _frag_conv_fwd('conv1x1_kres_fwd', x_nhwc, w_frag, bias, _ROWS_FRAG, int(stride), relu, tag)


def conv3x3_win_supported(h, w, cin, cout, kh, kw, stride, pad, dilation=(1, 1)):
    """True if this conv runs on the window-plane 3x3 kernel: stride 1, pad 1 on 28 / 14 / 7 pixel maps, or stride 2, pad 1 on
    56 / 28 / 14 pixel maps (h, w = the INPUT map)."""
    (sh, sw), (ph, pw) = _pair2(stride), _pair2(pad)
    if not host_policy.conv_win:      # A/B switch (tools/)
        return False
    if (kh, kw, ph, pw) != (3, 3, 1, 1) or tuple(dilation) != (1, 1):
        return False
    if (sh, sw) == (2, 2):
        return host_policy.conv_win_s2 and bool(lib().sc2_conv3x3s2_win_supported(h, w, cin, cout))
    return (sh, sw) == (1, 1) and \
        bool(lib().sc2_conv3x3_win_supported(h, w, cin, cout))   # (the caller checks the 2 GB operand bound: head._Conv.route)


def pack_conv_win(w):
    """[Cout, Cin, KH, KW] -> bf16 [Cin/32 * KH*KW][Cout/16][64][8], the weight stream of the window-plane kernels
    (sc2_conv3x3_win_fwd / sc2_conv2x2_win_fwd; layout: include/sc2_bottleneck.h): k-step = slab * KH*KW + tap, one MFMA
    operand fragment = 1 KB contiguous, output rows permuted so that a lane ends up with eight consecutive channels."""
    _dev(w, 'w')
    cout, cin, kh, kw = w.shape
    assert cout % 32 == 0 and cin % 32 == 0
    # cout = 32 g + 8 a + 4 j + b   (frow = 4 a + b);   cin = 32 cb + 8 fq + e
    g = w.detach().to(torch.bfloat16).reshape(cout // 32, 4, 2, 4, cin // 32, 4, 8, kh * kw)   # g, a, j, b, cb, fq, e, tap
    g = g.permute(4, 7, 0, 2, 5, 1, 3, 6)                                                   # cb, tap, g, j, fq, a, b, e
    return g.contiguous().reshape(cin // 32 * kh * kw, cout // 16, 64, 8)


def pack_conv3x3_win(w):
    """[Cout, Cin, 3, 3] -> bf16 [Cin/32 * 9][Cout/16][64][8] for sc2_conv3x3_win_fwd."""
    assert tuple(w.shape[2:]) == (3, 3)
    return pack_conv_win(w)


def conv2x2_win_supported(x_shape, cout, kh, kw, stride, pad):
    """True if this conv runs on the window-plane decoder kernel (k2, s1, Cout 256, width 56 / pad 0 or 55 / pad 1)."""
    (sh, sw), (ph, pw) = _pair2(stride), _pair2(pad)
    if not host_policy.conv2x2_win:      # A/B switch (tools/)
        return False
    N, H, W, Cin = x_shape
    if not _fits32(N * H * W * Cin, N * (H + 2 * ph - 1) * (W + 2 * pw - 1) * cout):
        return False
    return (kh, kw, sh, sw) == (2, 2, 1, 1) and ph == pw and bool(lib().sc2_conv2x2_win_supported(H, W, Cin, cout, ph))


def pack_conv2x2_win(w, gamma=None):
    """Weight stream of sc2_conv2x2_win_fwd: the conv's k-steps, then (fused GDN1) the effective gamma [256, 256] as a 1x1
    layer."""
    parts = [pack_conv_win(w)]
    if gamma is not None:
        assert tuple(gamma.shape) == (w.shape[0], w.shape[0])
        parts.append(pack_conv_win(gamma.reshape(gamma.shape[0], gamma.shape[1], 1, 1)))
    return torch.cat(parts).contiguous()


def conv2x2_win_tail_supported(x_shape):
    """True if the last decoder conv can take the head's first two 1x1 layers with it (55 x 55 input, sc2_conv2x2_win_tail_fwd)."""
    if not host_policy.conv2x2_win or not host_policy.w2_tail:      # A/B switches (tools/)
        return False
    N, H, W, Cin = x_shape
    if not _fits32(N * 56 * 56 * 256, N * H * W * Cin):
        return False
    return bool(lib().sc2_conv2x2_win_tail_supported(H, W, Cin))


def pack_conv2x2_win_tail(w, w1, wds):
    """Weight stream of sc2_conv2x2_win_tail_fwd: conv [256, Cin, 2, 2], then W1 [128, 256] (zero rows 128..255), then the two
    256-row halves of Wds [512, 256] as 1x1 layers."""
    assert tuple(w1.shape) == (128, 256) and tuple(wds.shape) == (512, 256) and w.shape[0] == 256
    w1p = torch.cat([w1, torch.zeros_like(w1)]).reshape(256, 256, 1, 1)
    parts = [pack_conv_win(w), pack_conv_win(w1p), pack_conv_win(wds[:256].reshape(256, 256, 1, 1)),
             pack_conv_win(wds[256:].reshape(256, 256, 1, 1))]
    return torch.cat(parts).contiguous()


def conv2x2_win_tail_fwd(x_nhwc, w_stream, bias1, bias_ds, want_y=False, tag=None):
    """-> (o1 [N,56,56,128], ods [N,28,28,512], y [N,56,56,256] or None); see include/sc2_bottleneck.h."""
    for t, name in ((x_nhwc, 'x'), (w_stream, 'w_stream'), (bias1, 'bias1'), (bias_ds, 'bias_ds')):
        _dev(t, name)
    assert x_nhwc.dtype == torch.bfloat16 and x_nhwc.dim() == 4 and x_nhwc.is_contiguous()
    N, H, W, Cin = x_nhwc.shape
    assert w_stream.dtype == torch.bfloat16 and w_stream.is_contiguous() and tuple(w_stream.shape) == (Cin // 32 * 4 + 24, 16, 64, 8)
    assert bias1.dtype == torch.float32 and bias1.numel() == 128 and bias_ds.dtype == torch.float32 and bias_ds.numel() == 512
    dev = x_nhwc.device
    o1 = torch.empty((N, 56, 56, 128), dtype=torch.bfloat16, device=dev)
    ods = torch.empty((N, 28, 28, 512), dtype=torch.bfloat16, device=dev)
    y = torch.empty((N, 56, 56, 256), dtype=torch.bfloat16, device=dev) if want_y else None
    with _timed(tag or 'conv2x2_win_tail'):
        _check(lib().sc2_conv2x2_win_tail_fwd(_ptr(x_nhwc), _ptr(w_stream), _ptr(bias1), _ptr(bias_ds), _ptr(y) if want_y else None,
                                              _ptr(o1), _ptr(ods), N, H, W, Cin, _stream()), 'conv2x2_win_tail_fwd')
    return o1, ods, y


def conv2x2_win_fwd(x_nhwc, w_frag, pad, beta=None, inverse=True, tag=None, out=None, channel0=0):
    """y = conv2x2(x, stride 1, pad) [-> GDN1 / inverse GDN1 when beta is given]; bf16 NHWC in / out, Cout 256.
    `out` [N, OH, OW, 512] with `channel0` 0 or 256: this launch's 256 channels go into that half of a 512-channel tensor (plain
    pad-1 convs only: the data gradient of a 512 -> 256 k2 layer is two such launches)."""
    for t, name in ((x_nhwc, 'x'), (w_frag, 'w_frag')):
        _dev(t, name)
    assert x_nhwc.dtype == torch.bfloat16 and x_nhwc.dim() == 4 and x_nhwc.is_contiguous()
    N, H, W, Cin = x_nhwc.shape
    fused = beta is not None
    assert w_frag.dtype == torch.bfloat16 and w_frag.is_contiguous() and \
        tuple(w_frag.shape) == (Cin // 32 * 4 + (8 if fused else 0), 16, 64, 8)
    if fused:
        _dev(beta, 'beta')
        assert beta.dtype == torch.float32 and beta.is_contiguous() and beta.numel() == 256
    pad = int(pad)
    if out is None:
        assert channel0 == 0
        out = torch.empty((N, H + 2 * pad - 1, W + 2 * pad - 1, 256), dtype=torch.bfloat16, device=x_nhwc.device)
    else:
        _dev(out, 'out')
        assert out.dtype == torch.bfloat16 and out.is_contiguous() and \
            tuple(out.shape) == (N, H + 2 * pad - 1, W + 2 * pad - 1, 512) and channel0 in (0, 256)
    with _timed(tag or 'conv2x2_win'):
        _check(lib().sc2_conv2x2_win_fwd(_ptr(x_nhwc), _ptr(w_frag), _ptr(beta) if fused else None, _ptr(out), N, H, W, Cin, pad,
                                         1 if fused else 0, 1 if inverse else 0, int(out.shape[3]), int(channel0), _stream()),
               'conv2x2_win_fwd')
    return out


def conv3x3_win_fwd(x_nhwc, w_frag, bias, relu=False, tag=None, stride=1, mask=None):
    """y = act(conv3x3(x, stride 1 or 2, pad 1) + bias); bf16 NHWC in / out; w_frag = pack_conv3x3_win(w).
    mask (stride 1, bf16 like y, no relu): y = mask > 0 ? conv + bias : 0 -- the gradient through a ReLU whose output is `mask`."""
    if int(stride) == 2:      # (an entry of its own, without a mask, for even maps: (H - 1) // 2 + 1 = H // 2)
        return _frag_conv_fwd('conv3x3s2_win_fwd', x_nhwc, w_frag, bias, _WIN_FRAG[9], 2, relu, tag, stride_arg=False)
    assert int(stride) == 1
    return _frag_conv_fwd('conv3x3_win_fwd', x_nhwc, w_frag, bias, _WIN_FRAG[9], 1, relu, tag, ('mask', mask), stride_arg=False)


def conv1x1_stream_supported(cin, cout, kh, kw, stride, pad):
    (sh, sw), (ph, pw) = _pair2(stride), _pair2(pad)
    if not host_policy.conv_stream:      # A/B switch (tools/)
        return False
    return kh == 1 and kw == 1 and sh == sw and ph == 0 and pw == 0 and \
        bool(lib().sc2_conv1x1_stream_supported(cin, cout, sh))


def conv1x1_stream_mask_supported(cin, cout, stride):
    return host_policy.conv_stream and bool(lib().sc2_conv1x1_stream_mask_supported(cin, cout, int(stride)))


def conv1x1_stream_fwd(x_nhwc, w_frag, bias, stride=1, residual=None, relu=False, tag=None, mask=None):
    """y = act(conv1x1(x) + bias [+ residual]) on the persistent streaming kernel; bf16 NHWC in / out."""
    return _frag_conv_fwd('conv1x1_stream_fwd', x_nhwc, w_frag, bias, _ROWS_FRAG, int(stride), relu, tag, ('residual', residual), ('mask', mask))


def conv1x1_pair_supported(k1, c, n2):
    """True if conv3 (k1 -> c, + residual + ReLU) of one Bottleneck block and conv1 (c -> n2, + ReLU) of the next run as one
    launch (sc2_conv1x1_pair_fwd); SC2_CONV1X1_PAIR=0: A/B switch."""
    return host_policy.conv1x1_pair and bool(lib().sc2_conv1x1_pair_supported(k1, c, n2))


def conv1x1_pair_fwd(o_nhwc, w3_frag, b3, identity, w1_frag, b1, tag=None):
    """h = relu(conv1x1(o; W3) + b3 + identity); u = relu(conv1x1(h; W1) + b1): -> (h [N,H,W,C], u [N,H,W,N2]), bf16 NHWC."""
    for t, name in ((o_nhwc, 'o'), (w3_frag, 'w3_frag'), (b3, 'b3'), (identity, 'identity'), (w1_frag, 'w1_frag'), (b1, 'b1')):
        _dev(t, name)
        assert t.is_contiguous(), name
    N, H, W, K1 = o_nhwc.shape
    C, N2 = w3_frag.shape[0] * 16, w1_frag.shape[0] * 16
    assert o_nhwc.dtype == torch.bfloat16 and identity.dtype == torch.bfloat16 and tuple(identity.shape) == (N, H, W, C)
    assert tuple(w3_frag.shape) == (C // 16, K1 // 32, 64, 8) and tuple(w1_frag.shape) == (N2 // 16, C // 32, 64, 8)
    assert b3.dtype == torch.float32 and b3.numel() == C and b1.dtype == torch.float32 and b1.numel() == N2
    h = torch.empty((N, H, W, C), dtype=torch.bfloat16, device=o_nhwc.device)
    u = torch.empty((N, H, W, N2), dtype=torch.bfloat16, device=o_nhwc.device)
    with _timed(tag or 'conv1x1_pair'):
        _check(lib().sc2_conv1x1_pair_fwd(_ptr(o_nhwc), _ptr(w3_frag), _ptr(b3), _ptr(identity), _ptr(h), _ptr(w1_frag), _ptr(b1),
                                          _ptr(u), N * H * W, K1, C, N2, _stream()), 'conv1x1_pair_fwd')
    return h, u


def conv2x2_c48_supported(x_shape, cout, kh, kw, stride, pad):
    """True if this conv runs on the streaming kernel of the FP encoder's last layer (Cin 48, k2, s1, p0, Cout <= 32)."""
    (sh, sw), (ph, pw) = _pair2(stride), _pair2(pad)
    if not host_policy.conv_c48:      # A/B switch (tools/)
        return False
    N, H, W, Cin = x_shape
    if not _fits32(N * H * W * Cin):
        return False
    return (kh, kw, sh, sw, ph, pw) == (2, 2, 1, 1, 0, 0) and bool(lib().sc2_conv2x2_c48_supported(H, W, Cin, cout))


def pack_conv2x2_c48(w):
    """[Cout <= 32, 48, 2, 2] -> bf16 fragment blocks [2][6][64][8] of W[co][kh*96 + kw*48 + ci] (rows >= Cout zero)."""
    _dev(w, 'w')
    cout = w.shape[0]
    assert tuple(w.shape[1:]) == (48, 2, 2) and cout <= 32
    w2d = torch.zeros((32, 192), dtype=torch.float32, device=w.device)
    w2d[:cout] = w.detach().float().permute(0, 2, 3, 1).reshape(cout, 192)
    return pack_weight_fragments(w2d)


def conv2x2_c48_fwd(x_nhwc, w_frag, cout, medians=None, tag=None, out=None):
    """x bf16 [N,H,W,48] -> f32 latent [N,cout,H-1,W-1], or (medians given) the int32 symbols round(y - median).
    `out`: a contiguous tensor of that dtype and element count to write into (e.g. a row block of a coder-group buffer)."""
    for t, name in ((x_nhwc, 'x'), (w_frag, 'w_frag')):
        _dev(t, name)
    assert x_nhwc.dtype == torch.bfloat16 and x_nhwc.dim() == 4 and x_nhwc.is_contiguous()
    N, H, W, Cin = x_nhwc.shape
    assert w_frag.dtype == torch.bfloat16 and w_frag.is_contiguous() and tuple(w_frag.shape) == (2, 6, 64, 8)
    sym = medians is not None
    if sym:
        _dev(medians, 'medians')
        assert medians.dtype == torch.float32 and medians.is_contiguous() and medians.numel() == cout
    dt = torch.int32 if sym else torch.float32
    if out is None:
        out = torch.empty((N, cout, H - 1, W - 1), dtype=dt, device=x_nhwc.device)
    else:
        _dev(out, 'out')
        assert out.dtype == dt and out.is_contiguous() and out.numel() == N * cout * (H - 1) * (W - 1)
        out = out.view(N, cout, H - 1, W - 1)
    with _timed(tag or 'conv2x2_c48'):
        _check(lib().sc2_conv2x2_c48_fwd(_ptr(x_nhwc), _ptr(w_frag), _ptr(medians) if sym else None, _ptr(out), N, H, W, Cin, cout,
                                         1 if sym else 0, _stream()), 'conv2x2_c48_fwd')
    return out


def conv1x1_win_supported(cin, cout, kh, kw, stride, pad):
    """True if this 1x1 conv can run on the window-plane 1x1 kernel (Cin, Cout multiples of 128, stride 1 or 2)."""
    (sh, sw), (ph, pw) = _pair2(stride), _pair2(pad)
    return (kh, kw, ph, pw) == (1, 1, 0, 0) and sh == sw and bool(lib().sc2_conv1x1_win_supported(cin, cout, sh))


def conv1x1_win_fwd(x_nhwc, w_frag, bias, stride=1, residual=None, relu=False, tag=None, mask=None):
    """y = act(conv1x1(x) + bias [+ residual]) on the window-plane 1x1 kernel; bf16 NHWC in / out;
    w_frag = pack_conv_win(w.reshape(Cout, Cin, 1, 1)).  mask (bf16 like y, no relu): y = mask > 0 ? value : 0."""
    return _frag_conv_fwd('conv1x1_win_fwd', x_nhwc, w_frag, bias, _WIN_FRAG[1], int(stride), relu, tag, ('residual', residual), ('mask', mask))


def conv1x1_w8_supported(cin, cout, kh, kw, stride, pad):
    """True if this 1x1 conv can run on the eight-wave 256-channel 1x1 kernel (Cin % 128 == 0, Cout % 256 == 0, stride 1 or 2)."""
    (sh, sw), (ph, pw) = _pair2(stride), _pair2(pad)
    return (kh, kw, ph, pw) == (1, 1, 0, 0) and sh == sw and bool(lib().sc2_conv1x1_w8_supported(cin, cout, sh))


def conv1x1_w8_fwd(x_nhwc, w_frag, bias, stride=1, residual=None, relu=False, tag=None, out=None):
    """y = act(conv1x1(x) + bias [+ residual]) on the eight-wave 256-channel 1x1 kernel (conv1x1_w8.hip); bf16 NHWC in / out;
    w_frag = pack_conv_win(w.reshape(Cout, Cin, 1, 1)), the stream of conv1x1_win_fwd, whose results it reproduces bit for bit.
    out: a contiguous bf16 tensor of the output's size to write into (default: a new one)."""
    return _frag_conv_fwd('conv1x1_w8_fwd', x_nhwc, w_frag, bias, _WIN_FRAG[1], int(stride), relu, tag, ('residual', residual), out=out)


def pack_gamma_fragments(gamma):
    """Effective gamma [C, C] (row = output channel) -> bf16 fragment-major [C/16][C/32][64][8]: entry
    (jt, ks, lane = fq*16 + frow, e) = gamma[jt*16 + frow, ks*32 + fq*8 + e], so that one MFMA operand fragment
    (16 channels x 32 k) is 1 KB contiguous.  Layout of the `gamma_frag` argument of sc2_conv2x2_gdn512_fwd."""
    _dev(gamma, 'gamma')
    C = gamma.shape[0]
    assert gamma.dim() == 2 and gamma.shape[1] == C and C % 32 == 0
    g = gamma.detach().to(torch.bfloat16).reshape(C // 16, 16, C // 32, 4, 8)      # jt, frow, ks, fq, e
    return g.permute(0, 2, 3, 1, 4).contiguous().reshape(C // 16, C // 32, 64, 8)


def conv2x2_gdn512_fwd(x_nhwc, w_packed, gamma_packed, beta, inverse, tag=None, want_t=False):
    """y = GDN1_512(conv2x2(x)) (s1, p1) in one launch; x bf16 [N,H,W,Cin] -> bf16 [N,H+1,W+1,512].
    gamma_packed: pack_gamma_fragments(effective gamma)."""
    for t, name in ((x_nhwc, 'x'), (w_packed, 'w_packed'), (gamma_packed, 'gamma_packed'), (beta, 'beta')):
        _dev(t, name)
    assert x_nhwc.dtype == torch.bfloat16 and x_nhwc.dim() == 4 and x_nhwc.is_contiguous()
    N, H, W, Cin = x_nhwc.shape
    assert w_packed.dtype == torch.bfloat16 and w_packed.is_contiguous() and w_packed.shape[0] == 512
    assert gamma_packed.dtype == torch.bfloat16 and gamma_packed.is_contiguous() and tuple(gamma_packed.shape) == (32, 16, 64, 8)
    assert beta.dtype == torch.float32 and beta.is_contiguous() and beta.numel() == 512
    out = torch.empty((N, H + 1, W + 1, 512), dtype=torch.bfloat16, device=x_nhwc.device)
    t = torch.empty_like(out) if want_t else None        # (training: the conv output in front of the GDN)
    with _timed(tag or 'conv2x2_gdn512'):
        _check(lib().sc2_conv2x2_gdn512_fwd(_ptr(x_nhwc), _ptr(w_packed), w_packed.shape[1], _ptr(gamma_packed), _ptr(beta),
                                            _ptr(out), _ptr(t), N, H, W, Cin, 1 if inverse else 0, _stream()), 'conv2x2_gdn512_fwd')
    return (out, t) if want_t else out


# --------------------------------------------------------------------------------------------- #
# entropy bottleneck
# --------------------------------------------------------------------------------------------- #
def eb_forward(y, params, mode, noise=None, lik_bound=1e-9, want_y_hat=True, want_nhwc=False, want_lik=True,
               want_bits=False):
    """y: f32 [N,C,*spatial] contiguous (NCHW). Returns (y_hat, y_hat_nhwc_bf16, lik, bits_partial)."""
    _dev(y, 'y')
    _dev(params, 'params')
    assert y.dtype == torch.float32 and y.is_contiguous() and params.dtype == torch.float32
    N, C = y.shape[0], y.shape[1]
    HW = y.numel() // (N * C)
    assert params.shape == (C, EB_PARAM_STRIDE) and params.is_contiguous()
    if noise is not None:
        _dev(noise, 'noise')
        assert noise.shape == y.shape and noise.dtype == torch.float32 and noise.is_contiguous()
    y_hat = torch.empty_like(y) if want_y_hat else None
    nhwc = torch.empty((N,) + tuple(y.shape[2:]) + (C,), dtype=torch.bfloat16, device=y.device) if want_nhwc else None
    lik = torch.empty_like(y) if want_lik else None
    nb = lib().sc2_eb_bits_partial_len(N, C, HW) if want_bits else 0
    bits = torch.empty((nb,), dtype=torch.float32, device=y.device) if want_bits else None
    _check(lib().sc2_eb_forward(_ptr(y), _ptr(noise), _ptr(params), N, C, HW, int(mode), float(lik_bound),
                                _ptr(y_hat), _ptr(nhwc), _ptr(lik), _ptr(bits), nb, _stream()), 'eb_forward')
    return y_hat, nhwc, lik, bits


def eb_backward(y, params, mode, noise, g_yhat, g_lik, lik_bound=1e-9):
    """Returns (g_y f32 like y, g_params f32 [C, 64]) -- the per-workgroup partial rows are summed here."""
    _dev(y, 'y')
    N, C = y.shape[0], y.shape[1]
    HW = y.numel() // (N * C)
    for t in (noise, g_yhat, g_lik):
        if t is not None:
            _dev(t, 'grad/noise')
            assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == y.numel()
    g_y = torch.empty_like(y)
    n_partial = lib().sc2_eb_bits_partial_len(N, C, HW)
    part = torch.empty((n_partial, EB_PARAM_STRIDE), dtype=torch.float32, device=y.device)
    _check(lib().sc2_eb_backward(_ptr(y), _ptr(noise), _ptr(params), N, C, HW, int(mode), float(lik_bound),
                                 _ptr(g_yhat), _ptr(g_lik), _ptr(g_y), _ptr(part), n_partial, _stream()),
           'eb_backward')
    g_params = part.view(N, C, n_partial // (N * C), EB_PARAM_STRIDE).sum(dim=(0, 2))
    return g_y, g_params


def eb_symbols(y, medians):
    _dev(y, 'y')
    _dev(medians, 'medians')
    assert y.dtype == torch.float32 and y.is_contiguous() and medians.dtype == torch.float32
    N, C = y.shape[0], y.shape[1]
    HW = y.numel() // (N * C)
    assert medians.numel() == C and medians.is_contiguous()
    sym = torch.empty(y.shape, dtype=torch.int32, device=y.device)
    _check(lib().sc2_eb_symbols(_ptr(y), _ptr(medians), N, C, HW, _ptr(sym), _stream()), 'eb_symbols')
    return sym


def eb_dequantize(symbols, medians, want_f32=True, want_nhwc=False):
    _dev(symbols, 'symbols')
    _dev(medians, 'medians')
    assert symbols.dtype == torch.int32 and symbols.is_contiguous()
    N, C = symbols.shape[0], symbols.shape[1]
    HW = symbols.numel() // (N * C)
    f32 = torch.empty(symbols.shape, dtype=torch.float32, device=symbols.device) if want_f32 else None
    nhwc = torch.empty((N,) + tuple(symbols.shape[2:]) + (C,), dtype=torch.bfloat16,
                       device=symbols.device) if want_nhwc else None
    _check(lib().sc2_eb_dequantize(_ptr(symbols), _ptr(medians), N, C, HW, _ptr(f32), _ptr(nhwc), _stream()),
           'eb_dequantize')
    return f32, nhwc


# --------------------------------------------------------------------------------------------- #
# GaussianConditional (hyperprior bottlenecks)
# --------------------------------------------------------------------------------------------- #
def _img_slice(t, ref, name):
    """f32 tensor with ref's shape that is dense inside each batch item (possibly a channel slice of a wider
    tensor, e.g. gaussian_params.chunk(2, 1)) -> (tensor, per-image element stride)."""
    _dev(t, name)
    assert t.dtype == torch.float32 and tuple(t.shape) == tuple(ref.shape), name
    if t.dim() < 2 or not t[0].is_contiguous():
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else t[0].numel())


def gc_forward(y, scales, means=None, noise=None, mode=EB_DEQUANTIZE, scale_bound=0.11, lik_bound=1e-9,
               want_y_hat=True, want_lik=True):
    """GaussianConditional.forward: y f32 [N,C,*spatial] contiguous -> (y_hat, likelihoods)."""
    _dev(y, 'y')
    assert y.dtype == torch.float32 and y.is_contiguous()
    N, chw = y.shape[0], y[0].numel()
    s_stride = m_stride = 0
    if scales is not None:
        scales, s_stride = _img_slice(scales, y, 'scales')
    if means is not None:
        means, m_stride = _img_slice(means, y, 'means')
    if noise is not None:
        _dev(noise, 'noise')
        assert noise.shape == y.shape and noise.dtype == torch.float32 and noise.is_contiguous()
    y_hat = torch.empty_like(y) if want_y_hat else None
    lik = torch.empty_like(y) if want_lik else None
    _check(lib().sc2_gc_forward(_ptr(y), _ptr(scales), s_stride, _ptr(means), m_stride, _ptr(noise), N, chw, int(mode),
                                float(scale_bound), float(lik_bound), _ptr(y_hat), _ptr(lik), _stream()), 'gc_forward')
    return y_hat, lik


def gc_backward(y, scales, means, noise, g_yhat, g_lik, scale_bound=0.11, lik_bound=1e-9):
    """Backward of gc_forward in noise mode -> (g_y, g_scales, g_means or None), dense f32 like y."""
    _dev(y, 'y')
    assert y.dtype == torch.float32 and y.is_contiguous()
    N, chw = y.shape[0], y[0].numel()
    scales, s_stride = _img_slice(scales, y, 'scales')
    m_stride = 0
    if means is not None:
        means, m_stride = _img_slice(means, y, 'means')
    for t in (noise, g_yhat, g_lik):
        if t is not None:
            _dev(t, 'grad/noise')
            assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == y.shape
    g_y, g_s = torch.empty_like(y), torch.empty_like(y)
    g_m = torch.empty_like(y) if means is not None else None
    _check(lib().sc2_gc_backward(_ptr(y), _ptr(scales), s_stride, _ptr(means), m_stride, _ptr(noise), N, chw,
                                 float(scale_bound), float(lik_bound), _ptr(g_yhat), _ptr(g_lik), _ptr(g_y), _ptr(g_s),
                                 _ptr(g_m), _stream()), 'gc_backward')
    return g_y, g_s, g_m


def gc_symbols_indexes(y, scales, means, scale_table, scale_bound=0.11, want_symbols=True, want_indexes=True):
    """-> (symbols int32 like y or None, indexes int32 like scales or None)."""
    ref = y if y is not None else scales
    _dev(ref, 'y')
    N, chw = ref.shape[0], ref[0].numel()
    s_stride = m_stride = 0
    if y is not None:
        assert y.dtype == torch.float32 and y.is_contiguous()
    if scales is not None:
        scales, s_stride = _img_slice(scales, ref, 'scales')
    if means is not None:
        means, m_stride = _img_slice(means, ref, 'means')
    n_table = 0
    if want_indexes:
        _dev(scale_table, 'scale_table')
        assert scale_table.dtype == torch.float32 and scale_table.is_contiguous()
        n_table = scale_table.numel()
    sym = torch.empty(ref.shape, dtype=torch.int32, device=ref.device) if want_symbols else None
    idx = torch.empty(ref.shape, dtype=torch.int32, device=ref.device) if want_indexes else None
    _check(lib().sc2_gc_symbols_indexes(_ptr(y), _ptr(scales), s_stride, _ptr(means), m_stride, N, chw,
                                        _ptr(scale_table) if want_indexes else None, n_table, float(scale_bound),
                                        _ptr(sym), _ptr(idx), _stream()), 'gc_symbols_indexes')
    return sym, idx


def gc_dequantize(symbols, means=None, want_f32=True, want_nhwc=False):
    """symbols int32 [N,C,*spatial] -> (y_hat f32 NCHW or None, y_hat bf16 NHWC or None); y_hat = symbols + means."""
    _dev(symbols, 'symbols')
    assert symbols.dtype == torch.int32 and symbols.is_contiguous() and symbols.dim() >= 3
    N, C = symbols.shape[0], symbols.shape[1]
    HW = symbols[0, 0].numel()
    m_stride = 0
    if means is not None:
        _dev(means, 'means')
        assert means.dtype == torch.float32 and tuple(means.shape) == tuple(symbols.shape)
        if not means[0].is_contiguous():
            means = means.contiguous()
        m_stride = means.stride(0) if N > 1 else means[0].numel()
    y_hat = torch.empty(symbols.shape, dtype=torch.float32, device=symbols.device) if want_f32 else None
    nhwc = torch.empty((N,) + tuple(symbols.shape[2:]) + (C,), dtype=torch.bfloat16, device=symbols.device) \
        if want_nhwc else None
    _check(lib().sc2_gc_dequantize(_ptr(symbols), _ptr(means), m_stride, N, C, HW, _ptr(y_hat), _ptr(nhwc), _stream()),
           'gc_dequantize')
    return y_hat, nhwc


# --------------------------------------------------------------------------------------------- #
# CDF + rANS
# --------------------------------------------------------------------------------------------- #
# --------------------------------------------------------------------------------------------- #
# element-wise pieces of the distillation step: csrc/loss.hip
# --------------------------------------------------------------------------------------------- #
def _same_dense_bf16(*ts):
    """True if the tensors are bf16 device tensors of one shape AND one dense memory layout (element i of each is the same
    logical element), so that an element-wise kernel may walk their storage linearly."""
    a = ts[0]
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.bfloat16 and t.shape == a.shape and
               t.stride() == a.stride() for t in ts):
        return False
    return (a.is_contiguous() or (a.dim() == 4 and a.is_contiguous(memory_format=torch.channels_last))) and a.numel() % 8 == 0


def mse_sum(x, y):
    """sum((x - y)^2) as an f32 device scalar; x, y: bf16, same shape and dense layout (_same_dense_bf16)."""
    assert _same_dense_bf16(x, y)
    n = x.numel()
    partial = torch.empty((int(lib().sc2_mse_partial_len(n)),), dtype=torch.float32, device=x.device)
    with _timed('mse_sum'):
        _check(lib().sc2_mse_sum_bf16(_ptr(x), _ptr(y), n, _ptr(partial), _stream()), 'mse_sum')
    return partial.double().sum().float()


def mse_grad(x, y, scale):
    """bf16(2 * scale * (x - y)) laid out like x; scale: f32 device scalar tensor."""
    assert _same_dense_bf16(x, y) and scale.is_cuda and scale.dtype == torch.float32 and scale.numel() == 1
    gx = torch.empty_like(x)
    with _timed('mse_grad'):
        _check(lib().sc2_mse_grad_bf16(_ptr(x), _ptr(y), x.numel(), _ptr(scale), _ptr(gx), _stream()), 'mse_grad')
    return gx


def relu_bwd(g, out, add=None):
    """(g [+ add]) * (out > 0), bf16, laid out like g (all operands one shape and dense layout)."""
    ops = (g, out) if add is None else (g, out, add)
    assert _same_dense_bf16(*ops)
    gi = torch.empty_like(g)
    with _timed('relu_bwd'):
        _check(lib().sc2_relu_bwd_bf16(_ptr(g), _ptr(out), _ptr(add), g.numel(), _ptr(gi), _stream()), 'relu_bwd')
    return gi


def relu_bwd_mse(g, out, t, scale, relu=True):
    """([g] + 2 * scale * (out - t)) [* (out > 0)], bf16 like out; g may be None; scale: f32 device scalar tensor."""
    ops = (out, t) if g is None else (g, out, t)
    assert _same_dense_bf16(*ops) and scale.is_cuda and scale.dtype == torch.float32 and scale.numel() == 1
    gi = torch.empty_like(out)
    with _timed('relu_bwd'):
        _check(lib().sc2_relu_bwd_mse_bf16(_ptr(g), _ptr(out), _ptr(t), _ptr(scale), out.numel(), 1 if relu else 0, _ptr(gi), _stream()),
               'relu_bwd_mse')
    return gi


# --------------------------------------------------------------------------------------------- #
# reference-precision (f32 operand) convolution / GDN1: csrc/conv_f32.hip
# --------------------------------------------------------------------------------------------- #
def nchw_f32_to_nhwc_f32(x, cpad=None):
    """x: f32 [N,C,H,W] -> f32 [N,H,W,Cpad] (channels >= C zero)."""
    _dev(x, 'x')
    assert x.dtype == torch.float32 and x.dim() == 4
    x = x.contiguous()
    N, C, H, W = x.shape
    cpad = (C + 3) // 4 * 4 if cpad is None else cpad
    y = torch.empty((N, H, W, cpad), dtype=torch.float32, device=x.device)
    _check(lib().sc2_nchw_f32_to_nhwc_f32(_ptr(x), _ptr(y), N, C, H, W, cpad, _stream()), 'nchw_f32_to_nhwc_f32')
    return y


def _precise_fused_gdn_supported(cout, chunk_channels):
    cout = int(cout)
    return cout <= 96 and (cout + 15) // 16 * 16 == int(chunk_channels(cout))


def conv_f32_fused_gdn_supported(cout):
    """conv + GDN1 in one f32 launch needs every channel of a pixel in one wave (Cout <= 96) AND a gamma stream as long as the
    chunk is wide: ceil(Cout / 16) * 16 == chunk width (96 / 48 / 32 / 20 ... yes; 64 or 16 no: two launches)."""
    return _precise_fused_gdn_supported(cout, lib().sc2_conv_f32_chunk_channels)


def _precise_weight_matrix(weight, cin_pad, chunk_channels, step_k):
    """Conv weight [Cout, Cin, KH, KW] -> (f32 [chunks * cc, steps * step_k] with k = (kh*KW + kw)*cin_pad + ci, zeros beyond Cout,
    Cin and K; chunks; NT = cc / 16; steps): the matrix whose elements pack_conv_f32 / pack_conv_split put into fragment order."""
    w = weight.detach().float()
    Cout, Cin, KH, KW = w.shape
    cin_pad = (Cin + 3) // 4 * 4 if cin_pad is None else cin_pad
    cc = int(chunk_channels(Cout))
    chunks = (Cout + cc - 1) // cc
    K = KH * KW * cin_pad
    steps = (K + step_k - 1) // step_k
    m = torch.zeros((chunks * cc, KH, KW, cin_pad), dtype=torch.float32, device=w.device)
    m[:Cout, :, :, :Cin] = w.permute(0, 2, 3, 1)
    return torch.nn.functional.pad(m.reshape(chunks * cc, K), (0, steps * step_k - K)), chunks, cc // 16, steps


def pack_conv_f32(weight, cin_pad=None):
    """Conv weight [Cout, Cin, KH, KW] (any float dtype) -> the f32 fragment-major stream of sc2_conv2d_f32_fwd:
    [chunks][steps][NT][64 lanes][4], entry (ch, s, nt, lane = q*16 + r, j) = W[ch*cc + nt*16 + r][16 s + 4 q + j] with
    k = (kh*KW + kw)*cin_pad + ci."""
    m, chunks, NT, steps = _precise_weight_matrix(weight, cin_pad, lib().sc2_conv_f32_chunk_channels, 16)
    m = m.reshape(chunks, NT, 16, steps, 4, 4)            # [ch, nt, r, s, q, j]
    return m.permute(0, 3, 1, 4, 2, 5).contiguous()       # [ch, s, nt, q, r, j]


def _precise_conv_setup(x_shape, device, cout, kh, kw, stride, padding, a_op, epilogue, out_format, ep_x, ep_beta, out, kpad=0, k_order=0,
                        scatter=None):
    """What conv2d_f32_fwd and conv2d_split_fwd share: x_shape (N, H, W, Cin) -> (the ConvDesc, the output tensor per out_format; a
    symbol buffer passed as `out` is used in place).  ep_x: the GDN operand [N,OH,OW,Cout] (with a fused epilogue: the f32 kernel's
    gamma fragments); ep_beta: [>= Cout]; both f32, dense.  stride / padding: int or (h, w) (the library takes a square stride only).
    scatter: (rows, cols, out f32 [N,out_H,out_W,cout], stride_h, stride_w, off_h, off_w) as for conv2d_fwd -- the launch computes
    rows x cols pixels per image and writes pixel (r, c) to (r*stride_h + off_h, c*stride_w + off_w) of `out`, which it returns."""
    N, H, W, Cin = x_shape
    (sh, sw), (ph, pw) = _pair2(stride), _pair2(padding)
    OH, OW = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    sc = (0, 0, 0, 0, 0, 0)
    if scatter is not None:
        OH, OW, y, s_h, s_w, o_h, o_w = scatter
        _dev(y, 'scatter output')
        # (the dtype and layout of `out` are the caller's promise whatever out_format says: the library refuses the formats it
        #  does not scatter)
        assert y.dtype == torch.float32 and y.is_contiguous() and y.dim() == 4 and y.shape[0] == N and y.shape[3] == cout
        sc = (y.shape[1], y.shape[2], s_h, s_w, o_h, o_w)
    d = ConvDesc(N=N, H=H, W=W, Cin=Cin, Cout=cout, KH=kh, KW=kw, stride_h=sh, stride_w=sw, pad_h=ph, pad_w=pw, OH=OH, OW=OW,
                 a_op=a_op, epilogue=epilogue, out_format=out_format, Kpad=kpad, Cout_pad=0, out_H=sc[0], out_W=sc[1], out_stride_h=sc[2],
                 out_stride_w=sc[3], out_off_h=sc[4], out_off_w=sc[5], k_order=k_order)
    if scatter is not None:
        pass
    elif out_format == OUT_F32_NHWC:
        y = torch.empty((N, OH, OW, cout), dtype=torch.float32, device=device)
    elif out_format == OUT_F32_NCHW:
        y = torch.empty((N, cout, OH, OW), dtype=torch.float32, device=device)
    else:
        assert out_format == OUT_I32_NCHW_SYM
        if out is not None:
            assert out.dtype == torch.int32 and out.is_contiguous() and out.numel() == N * cout * OH * OW
            y = out.view(N, cout, OH, OW)
        else:
            y = torch.empty((N, cout, OH, OW), dtype=torch.int32, device=device)
    for t in (ep_x, ep_beta):
        if t is not None:
            _dev(t, 'epilogue operand')
            assert t.dtype == torch.float32 and t.is_contiguous()
    if ep_x is not None and epilogue not in (EPI_FUSED_GDN, EPI_FUSED_IGDN):
        assert ep_x.numel() == N * OH * OW * cout
    if ep_beta is not None:
        assert ep_beta.numel() >= cout
    return d, y


def conv2d_f32_fwd(x_nhwc, w_frag, cout, kh, kw, stride, padding, a_op=AOP_NONE, epilogue=EPI_NONE, out_format=None,
                   ep_x=None, ep_beta=None, out=None, tag=None, cin_real=0, x_is_nchw_rgb=False, scatter=None):
    """x_nhwc: f32 [N,H,W,Cin] (Cin % 4 == 0) -> per out_format: OUT_F32_NHWC [N,OH,OW,Cout] (default), OUT_F32_NCHW
    [N,Cout,OH,OW], OUT_I32_NCHW_SYM int32 [N,Cout,OH,OW] (ep_beta = medians).  cin_real: the module's channel count when x_nhwc
    carries zero padding channels (3 of 4: the kernel skips the padding channel's products).  x_is_nchw_rgb: x_nhwc is the f32 NCHW
    image [N,3,H,W] itself (w_frag packed for cin_pad 4 as always): the kernel reads the three planes in place.
    padding: int or (h, w).  epilogue: also EPI_BIAS_RELU / EPI_BIAS_LEAKY_RELU (slope 0.01), ep_beta = the bias or None.
    scatter: see _precise_conv_setup (OUT_F32_NHWC, plain / bias / activation epilogues)."""
    _dev(x_nhwc, 'x')
    assert x_nhwc.dtype == torch.float32 and x_nhwc.dim() == 4 and x_nhwc.is_contiguous()
    assert w_frag.dtype == torch.float32 and w_frag.is_contiguous()
    out_format = OUT_F32_NHWC if out_format is None else out_format
    if x_is_nchw_rgb:
        N, c3, H, W = x_nhwc.shape
        assert c3 == 3
        Cin, cin_real = 4, 3
    else:
        N, H, W, Cin = x_nhwc.shape
    d, y = _precise_conv_setup((N, H, W, Cin), x_nhwc.device, cout, kh, kw, stride, padding, a_op, epilogue, out_format,
                               ep_x, ep_beta, out, kpad=int(cin_real or 0), k_order=1 if x_is_nchw_rgb else 0, scatter=scatter)
    with _timed(tag or 'conv_f32'):
        _check(lib().sc2_conv2d_f32_fwd(ctypes.byref(d), _ptr(x_nhwc), _ptr(w_frag), _ptr(y), _ptr(ep_x), _ptr(ep_beta),
                                        _stream()), 'conv2d_f32_fwd')
    return y


# --------------------------------------------------------------------------------------------- #
# split-bf16 convolution / GDN1 (f32 operands as sums of bf16 parts on the bf16 matrix cores): csrc/conv_split.hip
# --------------------------------------------------------------------------------------------- #
def conv_split_fused_gdn_supported(cout):
    """conv + GDN1 in one split launch: every channel of a pixel in one wave (Cout <= 96) and ceil(Cout / 16) * 16 == the chunk
    width (96 / 48 / 32 / 20 ... yes; 64 or 16 no: two launches)."""
    return _precise_fused_gdn_supported(cout, lib().sc2_conv_split_chunk_channels)


def split_bf16(t, ns):
    """f32 tensor -> ns bf16 tensors whose sum approximates t: hi = bf16(t), lo = bf16(t - hi), lo2 = bf16(t - hi - lo)."""
    parts, r = [], t.float().clone()
    for _ in range(ns):
        p = r.to(torch.bfloat16)
        parts.append(p)
        r = r - p.float()
    return parts


def pack_conv_split(weight, ns, cin_pad=None):
    """Conv weight [Cout, Cin, KH, KW] (any float dtype) -> the bf16 fragment stream of sc2_conv2d_split_fwd for ns (2 or 3) parts:
    [chunks][steps][ns][NT][64 lanes][8], entry (ch, s, part, nt, lane = q*16 + r, j) = part `part` of
    W[ch*cc + nt*16 + r][32 s + 16 (j >> 2) + 4 q + (j & 3)] with k = (kh*KW + kw)*cin_pad + ci."""
    ns = int(ns)
    if ns not in (2, 3):
        raise Sc2Error('pack_conv_split: ns must be 2 or 3, got {}'.format(ns))
    m, chunks, NT, steps = _precise_weight_matrix(weight, cin_pad, lib().sc2_conv_split_chunk_channels, 32)
    m = torch.stack(split_bf16(m, ns))                        # [part, row, k]
    m = m.reshape(ns, chunks, NT, 16, steps, 2, 4, 4)         # [part, ch, nt, r, s, half, q, e]
    return m.permute(1, 4, 0, 2, 6, 3, 5, 7).contiguous()     # [ch, s, part, nt, q, r, half, e]


def conv2d_split_fwd(x_nhwc, w_frag, cout, kh, kw, stride, padding, ns, a_op=AOP_NONE, epilogue=EPI_NONE, out_format=None,
                     ep_x=None, ep_beta=None, out=None, tag=None, cin_real=0, x_is_nchw_rgb=False, scatter=None):
    """conv2d_f32_fwd's interface on the split-bf16 kernels (ns = 2: three bf16 products per k, ns = 3: six; w_frag and, for the
    fused epilogues, ep_x = gamma from pack_conv_split with the same ns).  x_is_nchw_rgb: x_nhwc is the f32 NCHW image; it goes
    through its NHWC copy (same result).  cin_real is accepted and ignored (the padding channel's products are exact zeros)."""
    _dev(x_nhwc, 'x')
    assert x_nhwc.dtype == torch.float32 and x_nhwc.dim() == 4 and x_nhwc.is_contiguous()
    assert w_frag.dtype == torch.bfloat16 and w_frag.is_contiguous() and w_frag.dim() == 8 and w_frag.shape[2] == ns
    out_format = OUT_F32_NHWC if out_format is None else out_format
    if x_is_nchw_rgb:
        assert x_nhwc.shape[1] == 3
        x_nhwc = nchw_f32_to_nhwc_f32(x_nhwc, 4)
    N, H, W, Cin = x_nhwc.shape
    steps = (kh * kw * Cin + 31) // 32
    if w_frag.shape[1] != steps or w_frag.shape[0] * w_frag.shape[3] * 16 < cout:
        raise Sc2Error('conv2d_split_fwd: w_frag {} was not packed for Cout {} K {}'.format(tuple(w_frag.shape), cout, kh * kw * Cin))
    gamma = None
    if epilogue in (EPI_FUSED_GDN, EPI_FUSED_IGDN):
        gamma, ep_x = ep_x, None
        if gamma is not None:
            _dev(gamma, 'gamma')
            assert gamma.dtype == torch.bfloat16 and gamma.is_contiguous() and gamma.dim() == 8 and gamma.shape[2] == ns
            if gamma.shape[0] != 1 or gamma.shape[1] != (cout + 31) // 32 or gamma.shape[3] != w_frag.shape[3]:
                raise Sc2Error('conv2d_split_fwd: gamma {} was not packed as a 1x1 weight of {} channels'.format(tuple(gamma.shape), cout))
    d, y = _precise_conv_setup(tuple(x_nhwc.shape), x_nhwc.device, cout, kh, kw, stride, padding, a_op, epilogue, out_format,
                               ep_x, ep_beta, out, scatter=scatter)
    with _timed(tag or 'conv_split'):
        _check(lib().sc2_conv2d_split_fwd(ctypes.byref(d), int(ns), _ptr(x_nhwc), _ptr(w_frag), _ptr(y), _ptr(ep_x), _ptr(gamma),
                                          _ptr(ep_beta), _stream()), 'conv2d_split_fwd')
    return y


def pmf_to_quantized_cdf(pmf, precision=16):
    """Host function. pmf: sequence / 1-D CPU tensor of floats -> torch.IntTensor (len+1)."""
    if isinstance(pmf, torch.Tensor):
        pmf = pmf.detach().cpu().tolist()
    n = len(pmf)
    arr = (ctypes.c_float * n)(*pmf)
    out = (ctypes.c_uint32 * (n + 1))()
    _check(lib().sc2_pmf_to_quantized_cdf(arr, n, int(precision), out), 'pmf_to_quantized_cdf')
    return torch.IntTensor(list(out))


def rans_max_bytes(n_sym):
    return int(lib().sc2_rans_max_bytes(int(n_sym)))


# ---- host range coder (csrc/rans_host.cpp): a few streams are coded faster by CPU cores than by GPU lanes ----------------
def host_coder_max_streams():
    """Stream count up to which compress() / decompress() use the library's HOST coder (0 = always the device coder)."""
    # measured (profiles/r03c_*): the device coder takes ~120 ns per symbol of ONE stream however few streams there are (one
    # lane each), a host thread ~15-25 ns; with up to 32 threads the host wins far beyond a handful of streams (16 streams
    # of 393 k symbols, the 513 x 513 batch: 85 ms on the device coder)
    return int(host_policy.host_coder_max_streams)


class HostRansTables(object):
    """Prepared CDF tables of the host coder (opaque handle of sc2_rans_host_tables_create), built from int32 tensors /
    arrays `cdfs` [n_cdfs, stride], `cdf_sizes` [n_cdfs], `offsets` [n_cdfs] wherever they live."""

    def __init__(self, cdfs, cdf_sizes, offsets):
        import numpy as np
        to_np = lambda t: np.ascontiguousarray((t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)), dtype=np.int32)  # noqa: E731
        c, z, o = to_np(cdfs), to_np(cdf_sizes).reshape(-1), to_np(offsets).reshape(-1)
        assert c.ndim == 2 and z.shape[0] == c.shape[0] == o.shape[0]
        self.n_cdfs = int(c.shape[0])
        self._h = ctypes.c_void_p(0)
        _check(lib().sc2_rans_host_tables_create(c.ctypes.data, c.shape[0], c.shape[1], z.ctypes.data, o.ctypes.data,
                                                 ctypes.byref(self._h)), 'rans_host_tables_create')

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h and _lib is not None:
            _lib.sc2_rans_host_tables_destroy(h)


def host_cores():
    """CPUs this process may reasonably load: its affinity mask, and -- under a launcher that starts several ranks on the node
    (LOCAL_WORLD_SIZE) -- no more than its share of the machine (eight ranks each spawning a coder thread per CPU of the node would
    oversubscribe it eightfold)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    try:
        ranks = max(1, int(os.environ.get('LOCAL_WORLD_SIZE', '1')))
    except ValueError:
        ranks = 1
    return max(1, min(n, (os.cpu_count() or n) // ranks))


def _host_threads(n_streams, cap=32):
    return max(1, min(int(n_streams), host_cores(), cap))


def rans_code_host(tables, symbols, index_div, dec_out, out_stride=None, threads=None, scratch=None):
    """HOST encode + decode of every row of `symbols` (int32 numpy [n_streams, n_sym], implicit indexes) in one library call;
    the decoded symbols land in `dec_out` (int32 numpy of the same shape, e.g. a view of a pinned tensor).
    -> (buf uint8 [n_streams, stride], offset, nbytes, status) numpy; status = encode | decode bits.
    `scratch`: a dict that keeps the 37 MB of byte rows between calls -- a fresh allocation is first touched by the coder's threads,
    one page fault per 4 KB under the process's memory-map lock: 3 - 4 ms of a 5 ms call on a 128-core host."""
    import numpy as np
    n_streams, n_sym = symbols.shape
    assert symbols.dtype == np.int32 and symbols.flags['C_CONTIGUOUS'] and dec_out.dtype == np.int32 and dec_out.flags['C_CONTIGUOUS']
    assert dec_out.shape == symbols.shape
    if out_stride is None:
        out_stride = 2 * n_sym + 64
    out_stride = (int(out_stride) + 3) // 4 * 4
    key = ('rows', n_streams, out_stride)
    if scratch is not None and key in scratch:
        buf = scratch[key]
    else:
        buf = np.empty((n_streams, out_stride // 4), dtype=np.uint32)
        if scratch is not None:
            buf.fill(0)         # (touch the pages once, here)
            scratch[key] = buf
    off = np.empty((n_streams,), dtype=np.int32)
    nb = np.empty((n_streams,), dtype=np.int32)
    st = np.empty((n_streams,), dtype=np.int32)
    n_thr = int(threads) if threads else _host_threads(n_streams, cap=64)
    _check(lib().sc2_rans_code_host(tables._h, symbols.ctypes.data, None, int(index_div), n_streams, n_sym, buf.ctypes.data, out_stride,
                                    off.ctypes.data, nb.ctypes.data, dec_out.ctypes.data, st.ctypes.data, n_thr), 'rans_code_host')
    return buf.view(np.uint8).reshape(n_streams, out_stride), off, nb, st


def clock_probe(n_workgroups=16, n_samples=64, period_us=20.0, stream=None):
    """DIAGNOSTIC (csrc/diag.hip): launches the clock probe on `stream` (default: the current one) and returns the int64 tensor
    [n_workgroups, n_samples, 3] = (s_memtime, s_memrealtime, XCC id) it fills; read it after a synchronize."""
    out = torch.zeros((n_workgroups, n_samples, 3), dtype=torch.int64, device='cuda')
    s = ctypes.c_void_p(stream.cuda_stream) if stream is not None else _stream()
    _check(lib().sc2_clock_probe(_ptr(out), n_workgroups, n_samples, int(round(period_us * 100.0)), s), 'clock_probe')
    return out


def rans_encode_host(tables, symbols, indexes=None, index_div=0, out_stride=None):
    """symbols: int32 numpy [n_streams, n_sym] (HOST) -> (list[bytes], status int32 numpy [n_streams])."""
    import numpy as np
    symbols = np.ascontiguousarray(symbols, dtype=np.int32)
    n_streams, n_sym = symbols.shape
    if indexes is not None:
        indexes = np.ascontiguousarray(indexes, dtype=np.int32)
        assert indexes.shape == symbols.shape
    if out_stride is None:
        out_stride = 2 * n_sym + 64
    out_stride = (int(out_stride) + 3) // 4 * 4
    buf = np.empty((n_streams, out_stride // 4), dtype=np.uint32)
    off = np.empty((n_streams,), dtype=np.int32)
    nb = np.empty((n_streams,), dtype=np.int32)
    st = np.empty((n_streams,), dtype=np.int32)
    _check(lib().sc2_rans_encode_host(tables._h, symbols.ctypes.data, indexes.ctypes.data if indexes is not None else None,
                                      int(index_div), n_streams, n_sym, buf.ctypes.data, out_stride, off.ctypes.data,
                                      nb.ctypes.data, st.ctypes.data, _host_threads(n_streams)), 'rans_encode_host')
    raw = buf.view(np.uint8).reshape(n_streams, out_stride)
    return [raw[i, int(off[i]):int(off[i]) + int(nb[i])].tobytes() for i in range(n_streams)], st


def rans_decode_host(tables, strings, n_sym, indexes=None, index_div=0):
    """strings: list[bytes] -> (int32 numpy [n_streams, n_sym] (HOST), status int32 numpy [n_streams])."""
    import numpy as np
    n_streams = len(strings)
    stride = (max([len(q) for q in strings] + [8]) + 3) // 4 * 4
    buf = np.zeros((n_streams, stride // 4), dtype=np.uint32)
    raw = buf.view(np.uint8).reshape(n_streams, stride)
    nb = np.empty((n_streams,), dtype=np.int32)
    for i, q in enumerate(strings):
        raw[i, :len(q)] = np.frombuffer(q, dtype=np.uint8)
        nb[i] = len(q)
    off = np.zeros((n_streams,), dtype=np.int32)
    if indexes is not None:
        indexes = np.ascontiguousarray(indexes, dtype=np.int32)
        assert indexes.shape == (n_streams, n_sym)
    sym = np.empty((n_streams, int(n_sym)), dtype=np.int32)
    st = np.empty((n_streams,), dtype=np.int32)
    _check(lib().sc2_rans_decode_host(tables._h, buf.ctypes.data, stride, off.ctypes.data, nb.ctypes.data,
                                      indexes.ctypes.data if indexes is not None else None, int(index_div), n_streams,
                                      int(n_sym), sym.ctypes.data, st.ctypes.data, _host_threads(n_streams)), 'rans_decode_host')
    return sym, st


def rans_encode_batch(symbols, cdfs, cdf_sizes, offsets, indexes=None, index_div=0, out_stride=None):
    """symbols: i32 [n_streams, n_sym] (device).  Returns (buf u8 [n_streams, stride], offset, nbytes, status)."""
    _dev(symbols, 'symbols')
    for name, t in (('cdfs', cdfs), ('cdf_sizes', cdf_sizes), ('offsets', offsets)):
        _dev(t, name)
        assert t.dtype == torch.int32 and t.is_contiguous(), name
    assert symbols.dtype == torch.int32 and symbols.dim() == 2 and symbols.is_contiguous()
    n_streams, n_sym = symbols.shape
    if indexes is not None:
        _dev(indexes, 'indexes')
        assert indexes.shape == symbols.shape and indexes.dtype == torch.int32 and indexes.is_contiguous()
    if out_stride is None:
        out_stride = 2 * n_sym + 64  # 16 bits / symbol + flush; overflow is reported via status
    out_stride = (int(out_stride) + 3) // 4 * 4
    dev = symbols.device
    buf = torch.empty((n_streams, out_stride), dtype=torch.uint8, device=dev)
    off = torch.empty((n_streams,), dtype=torch.int32, device=dev)
    nb = torch.empty((n_streams,), dtype=torch.int32, device=dev)
    st = torch.empty((n_streams,), dtype=torch.int32, device=dev)
    ws_bytes = int(lib().sc2_rans_workspace_bytes(n_streams, n_sym, cdfs.shape[0], cdfs.shape[1]))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    with _timed('rans_encode' if indexes is None else 'rans_encode.indexed'):   # (.indexed: per-symbol CDF rows, the hyperprior's y stream)
        _check(lib().sc2_rans_encode_batch(_ptr(symbols), _ptr(indexes), int(index_div), n_streams, n_sym, _ptr(cdfs),
                                       cdfs.shape[0], cdfs.shape[1], _ptr(cdf_sizes), _ptr(offsets), _ptr(buf),
                                         out_stride, _ptr(off), _ptr(nb), _ptr(st), _ptr(ws), ws_bytes, _stream()),
               'rans_encode_batch')
    return buf, off, nb, st


def rans_decode_dequantize_batch(buf, off, nb, n_sym, cdfs, cdf_sizes, offsets, index_div, medians, want_symbols=False):
    """Decode (implicit indexes: row = position // index_div) with the dequantisation fused into the last pass:
    -> (y_hat bf16 NHWC [n_streams, index_div, C] flat pixels, status, symbols or None)."""
    for name, t in (('buf', buf), ('off', off), ('nb', nb), ('cdfs', cdfs), ('cdf_sizes', cdf_sizes), ('offsets', offsets),
                    ('medians', medians)):
        _dev(t, name)
        assert t.is_contiguous(), name
    assert buf.dtype == torch.uint8 and buf.dim() == 2 and medians.dtype == torch.float32
    n_streams, stride = buf.shape
    C = cdfs.shape[0]
    assert medians.numel() == C and n_sym == C * int(index_div)
    dev = buf.device
    y_hat = torch.empty((n_streams, int(index_div), C), dtype=torch.bfloat16, device=dev)
    sym = torch.empty((n_streams, n_sym), dtype=torch.int32, device=dev) if want_symbols else None
    st = torch.empty((n_streams,), dtype=torch.int32, device=dev)
    ws_bytes = int(lib().sc2_rans_workspace_bytes(n_streams, n_sym, cdfs.shape[0], cdfs.shape[1]))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    # the last pass of the call (dequantise + NHWC transposition) is EntropyModel.dequantize of the reference's decode: an active
    # KernelTimer that selects 'dec.dequantize' gets its own event pair around it (recorded by the library on this stream)
    t = KernelTimer.active
    ev = None
    if t is not None and (t.select is None or t.select('dec.dequantize')):
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        for e in ev:
            e.record()         # creates the hipEvent_t; the library records it again where it belongs
        t.records.append(('dec.dequantize', ev[0], ev[1], n_streams))
    with _timed('rans_decode'):
        _check(lib().sc2_rans_decode_dequantize_batch_ev(_ptr(buf), stride, _ptr(off), _ptr(nb), int(index_div), n_streams, int(n_sym),
                                                         _ptr(cdfs), cdfs.shape[0], cdfs.shape[1], _ptr(cdf_sizes), _ptr(offsets),
                                                         _ptr(medians), _ptr(sym) if want_symbols else None, _ptr(y_hat), _ptr(st),
                                                         _ptr(ws), ws_bytes, _stream(),
                                                         ctypes.c_void_p(ev[0].cuda_event) if ev else None,
                                                         ctypes.c_void_p(ev[1].cuda_event) if ev else None),
               'rans_decode_dequantize_batch')
    return y_hat, st, sym


def rans_decode_dequantize_supported(n_cdfs, cdf_stride):
    """True if sc2_rans_decode_dequantize_batch takes these tables (channel count % 8 == 0, <= 64, rows within the LUT decoder)."""
    return n_cdfs % 8 == 0 and n_cdfs <= 64 and cdf_stride <= 4096 and host_policy.rans_fused_dq


# sc2_rans_decode_path: enum sc2_rans_dec_path / sc2_rans_dec_finish of include/sc2_bottleneck.h by name
RANS_DEC_PATHS = {1: 'lut8', 2: 'lut-u8', 3: 'lut-u16', 4: 'ragged2', 5: 'ragged-8bit', 6: 'ragged-5bit', 7: 'generic-lds', 8: 'generic-global'}
RANS_DEC_FINISHES = {0: 'none', 1: 'transpose', 2: 'dq-reg', 3: 'dq-lds'}


def rans_decode_path(explicit_indexes, index_div, n_streams, n_sym, n_cdfs, cdf_stride, fused_dq=False):
    """Which kernels a decode call of these sizes runs under the policy in force (no launch): -> (serial kernel, waves per workgroup,
    finishing pass) by the names above; the decision the decode entry points switch on."""
    waves, finish = ctypes.c_int32(0), ctypes.c_int32(0)
    path = int(lib().sc2_rans_decode_path(int(bool(explicit_indexes)), int(index_div), int(n_streams), int(n_sym), int(n_cdfs), int(cdf_stride),
                                          int(bool(fused_dq)), ctypes.byref(waves), ctypes.byref(finish)))
    if path not in RANS_DEC_PATHS:
        raise Sc2Error('rans_decode_path: no decode call takes these sizes')
    return RANS_DEC_PATHS[path], waves.value, RANS_DEC_FINISHES[finish.value]


def rans_decode_batch(buf, off, nb, n_sym, cdfs, cdf_sizes, offsets, indexes=None, index_div=0):
    """buf: u8 [n_streams, stride] (device), stream i at buf[i, off[i]:off[i]+nb[i]].  Returns (symbols, status)."""
    for name, t in (('buf', buf), ('off', off), ('nb', nb), ('cdfs', cdfs), ('cdf_sizes', cdf_sizes),
                    ('offsets', offsets)):
        _dev(t, name)
        assert t.is_contiguous(), name
    assert buf.dtype == torch.uint8 and buf.dim() == 2
    n_streams, stride = buf.shape
    dev = buf.device
    sym = torch.empty((n_streams, n_sym), dtype=torch.int32, device=dev)
    st = torch.empty((n_streams,), dtype=torch.int32, device=dev)
    if indexes is not None:
        _dev(indexes, 'indexes')
        assert indexes.shape == sym.shape and indexes.dtype == torch.int32 and indexes.is_contiguous()
    ws_bytes = int(lib().sc2_rans_workspace_bytes(n_streams, n_sym, cdfs.shape[0], cdfs.shape[1]))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    with _timed('rans_decode' if indexes is None else 'rans_decode.indexed'):
        _check(lib().sc2_rans_decode_batch(_ptr(buf), stride, _ptr(off), _ptr(nb), _ptr(indexes), int(index_div),
                                       n_streams, int(n_sym), _ptr(cdfs), cdfs.shape[0], cdfs.shape[1],
                                       _ptr(cdf_sizes), _ptr(offsets), _ptr(sym), _ptr(st), _ptr(ws), ws_bytes,
                                           _stream()), 'rans_decode_batch')
    return sym, st


# --------------------------------------------------------------------------------------------- #
# serial context-model scan (ar_context.hip): the joint autoregressive hierarchical prior's compress / decompress
# --------------------------------------------------------------------------------------------- #
def ar_scan(weights, p1, y_hat_pad, y_hat_nhwc, scale_table, scale_bound, y=None, symbols=None, indexes=None, decode=None,
            pix=None, gaussian_params=None):
    """One scan over pixels pix = (pix0, pix1) of the B x H x W latent (all of it by default).

    weights: dict wc / bc / w1 / w2 / b2 / w3 / b3 (k-major matrices, f32 biases; see sc2_ar_scan_args); the four matrices are
    all bf16 (sc2_ar_scan) or all f32 (sc2_ar_scan_f32, timing tags ar_scan.enc.f32 / ar_scan.dec.f32): the dtype routes, and a
    mixed dict raises Sc2Error before any launch.  p1: f32 [B,H,W,C1p];
    y_hat_pad: f32 [B,H+2,W+4,M] (updated in place); y_hat_nhwc: bf16 [B,H,W,M] or None.
    Encoder: y f32 [B,M,H,W], symbols / indexes i32 [B,H*W*M] (written).  Decoder: decode = dict buf / off / nb / cdfs /
    cdf_sizes / offsets / cdf_entries / st_x / st_pos / status (device tensors; state updated in place), symbols optional.
    gaussian_params: None or f32 [B,H*W,2M] receiving each pixel's scales and means."""
    B, H, W, C1p = p1.shape
    M = y_hat_pad.shape[3]
    assert tuple(y_hat_pad.shape) == (B, H + 2, W + 4, M) and y_hat_pad.dtype == torch.float32 and y_hat_pad.is_contiguous()
    assert p1.dtype == torch.float32 and p1.is_contiguous()
    C2p = weights['w2'].shape[1]
    wdtypes = set(weights[name].dtype for name in ('wc', 'w1', 'w2', 'w3'))
    if len(wdtypes) != 1 or not wdtypes <= {torch.bfloat16, torch.float32}:
        raise Sc2Error('ar_scan: wc / w1 / w2 / w3 must be all bf16 or all f32, got {}'.format(
            ', '.join('{} {}'.format(name, weights[name].dtype) for name in ('wc', 'w1', 'w2', 'w3'))))
    wdtype = wdtypes.pop()
    for name in ('wc', 'bc', 'w1', 'w2', 'b2', 'w3', 'b3'):
        t = _dev(weights[name], name)
        assert t.is_contiguous() and t.dtype == (wdtype if name[0] == 'w' else torch.float32), name
    assert tuple(weights['wc'].shape) == (12 * M, 2 * M) and tuple(weights['w1'].shape) == (2 * M, C1p)
    assert tuple(weights['w2'].shape) == (C1p, C2p) and tuple(weights['w3'].shape) == (C2p, 2 * M)
    for t in (p1, y_hat_pad, scale_table):
        _dev(t, 'tensor')
    assert scale_table.dtype == torch.float32 and scale_table.is_contiguous()
    if y_hat_nhwc is not None:
        assert tuple(y_hat_nhwc.shape) == (B, H, W, M) and y_hat_nhwc.dtype == torch.bfloat16 and y_hat_nhwc.is_contiguous()
    for t in (symbols, indexes):
        if t is not None:
            _dev(t, 'symbols / indexes')
            assert tuple(t.shape) == (B, H * W * M) and t.dtype == torch.int32 and t.is_contiguous()
    pix0, pix1 = (0, H * W) if pix is None else pix
    a = ArScanArgs()
    a.B, a.H, a.W, a.M, a.C1p, a.C2p = B, H, W, M, C1p, C2p
    a.n_table, a.pix0, a.pix1 = scale_table.numel(), pix0, pix1
    a.scale_bound = float(scale_bound)
    for name in ('wc', 'bc', 'w1', 'w2', 'b2', 'w3', 'b3'):
        setattr(a, name, weights[name].data_ptr())
    a.p1, a.scale_table, a.y_hat_pad = p1.data_ptr(), scale_table.data_ptr(), y_hat_pad.data_ptr()
    a.y_hat_nhwc = y_hat_nhwc.data_ptr() if y_hat_nhwc is not None else None
    a.symbols = symbols.data_ptr() if symbols is not None else None
    a.indexes = indexes.data_ptr() if indexes is not None else None
    if gaussian_params is not None:
        _dev(gaussian_params, 'gaussian_params')
        assert tuple(gaussian_params.shape) == (B, H * W, 2 * M) and gaussian_params.dtype == torch.float32
        assert gaussian_params.is_contiguous()
        a.gaussian_params = gaussian_params.data_ptr()
    if decode is None:
        _dev(y, 'y')
        assert tuple(y.shape) == (B, M, H, W) and y.dtype == torch.float32 and y.is_contiguous()
        a.y = y.data_ptr()
    else:
        d = decode
        assert d['buf'].dtype == torch.uint8 and d['buf'].dim() == 2 and d['buf'].shape[0] == B
        assert d['cdfs'].dtype == torch.int32 and d['cdfs'].dim() == 2 and d['cdfs'].shape[0] == scale_table.numel()
        assert d['st_x'].dtype == torch.int64 and d['st_x'].numel() == B
        for name in ('buf', 'off', 'nb', 'cdfs', 'cdf_sizes', 'offsets', 'st_x', 'st_pos', 'status'):
            _dev(d[name], name)
            assert d[name].is_contiguous(), name
        a.decode = 1
        a.stride = d['buf'].shape[1]
        a.n_cdfs, a.cdf_stride, a.cdf_entries = d['cdfs'].shape[0], d['cdfs'].shape[1], int(d['cdf_entries'])
        for name, key in (('buf', 'buf'), ('io_offset', 'off'), ('io_nbytes', 'nb'), ('cdfs', 'cdfs'),
                          ('cdf_sizes', 'cdf_sizes'), ('offsets', 'offsets'), ('st_x', 'st_x'), ('st_pos', 'st_pos'),
                          ('status', 'status')):
            setattr(a, name, d[key].data_ptr())
    f32 = wdtype == torch.float32
    with _timed('ar_scan.{}{}'.format('dec' if decode is not None else 'enc', '.f32' if f32 else '')):
        _check((lib().sc2_ar_scan_f32 if f32 else lib().sc2_ar_scan)(ctypes.byref(a), _stream()), 'ar_scan')


def rans_decode_resume(buf, off, nb, indexes, cdfs, cdf_sizes, offsets, state=None, last=True):
    """Decodes indexes.shape[1] more symbols of every stream (explicit per-symbol indexes), continuing from `state`
    (st_x i64 [N], st_pos i32 [N], status i32 [N]; None: start at each stream's first word).  -> (symbols, state); the
    state's status carries the stream's error bits (4: an index outside the table, row 0 decoded in its place; 8: corrupt /
    truncated; 16: `last` and the stream did not end there); 4 and 8 stay set in the calls that continue the stream."""
    for name, t in (('buf', buf), ('off', off), ('nb', nb), ('indexes', indexes), ('cdfs', cdfs), ('cdf_sizes', cdf_sizes),
                    ('offsets', offsets)):
        _dev(t, name)
        assert t.is_contiguous(), name
    assert buf.dtype == torch.uint8 and buf.dim() == 2 and indexes.dtype == torch.int32 and indexes.dim() == 2
    n, stride = buf.shape
    dev = buf.device
    first = state is None
    if first:
        state = (torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                 torch.zeros(n, dtype=torch.int32, device=dev))
    sym = torch.empty_like(indexes)
    with _timed('rans_decode_resume'):
        _check(lib().sc2_rans_decode_resume(_ptr(buf), stride, _ptr(off), _ptr(nb), _ptr(indexes), n, indexes.shape[1],
                                            _ptr(cdfs), cdfs.shape[0], cdfs.shape[1], _ptr(cdf_sizes), _ptr(offsets),
                                            int(first), int(bool(last)), _ptr(state[0]), _ptr(state[1]), _ptr(state[2]),
                                            _ptr(sym), _stream()), 'rans_decode_resume')
    return sym, state
