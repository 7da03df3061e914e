"""ctypes binding of libsiammask_hip.so (the C ABI in include/siammask_hip.h).

``import torch`` happens before ``ctypes.CDLL`` on purpose: torch bundles a HIP runtime with
the same SONAME (libamdhip64.so.7) as /opt/rocm's, and loading torch first makes the
dynamic linker resolve the library's dependency to the runtime torch already uses, so that
streams and device pointers are shared.

The product path has no CPU fallback: if the shared library is missing, loading raises.
"""
import ctypes
import os
import subprocess

import torch  # noqa: F401  (must precede CDLL, see above)

_HERE = os.path.dirname(os.path.abspath(__file__))
# SMK_LIB=<path>: load another build of the library (measurement aid: A/B arms of compile-time choices, tools/measure/build_variant.sh)
LIB_PATH = os.environ.get("SMK_LIB") or os.path.join(_HERE, "libsiammask_hip.so")
CSRC = os.path.join(_HERE, "csrc")

DTYPE = {"f32": 0, "fp32": 0, "float32": 0, "f16": 1, "fp16": 1, "float16": 1, "half": 1,
         "f16x3": 2}       # split-operand fp16 (SMK_DTYPE_F16X3): fp32-grade cls / loc / box on the fp16 matrix pipe
VARIANT = {"rpn": 0, "base": 1, "sharp": 2}
TRACK_BOX, TRACK_MASK, TRACK_NO_MASK_HEAD = 0, 1, 2
HP_STRIDE = 4     # SMK_HP_STRIDE: columns of a per-stream hp table (penalty_k, window_influence, lr, reserved 0)

# every symbol include/siammask_hip.h declares
SYMBOLS = (
    "smk_version", "smk_last_error", "smk_create", "smk_destroy", "smk_set_weight",
    "smk_finalize_weights", "smk_template", "smk_track", "smk_refine", "smk_set_decode_params", "smk_decode", "smk_step", "smk_set_graph_mode", "smk_seq_status", "smk_seq_sync_check", "smk_set_result_ring", "smk_result_ring_cursor", "smk_set_pipeline", "smk_pipeline_join", "smk_pipeline_observe",
    "smk_debug_read", "smk_debug_seq_inject", "smk_tune", "smk_tune_get", "smk_profile", "smk_profile_dump", "smk_op_conv2d_ex", "smk_op_conv2d", "smk_op_dw_xcorr",
    "smk_op_maxpool3x3s2", "smk_op_stem_pool", "smk_op_l1_block", "smk_op_conv_seq", "smk_host_conv2d_ex", "smk_host_plan_conv", "smk_host_plan_seq", "smk_host_arena_elems", "smk_host_chain_rows", "smk_bench_conv", "smk_packed_size", "smk_export_packed",
    "smk_import_packed", "smk_crop_resize", "smk_paste_mask", "smk_paste_labels", "smk_mask_rbox_workspace", "smk_mask_rbox",
    "smk_trk_state_bytes", "smk_trk_set", "smk_trk_plan", "smk_trk_advance", "smk_crop_resize_dev", "smk_paste_mask_dev",
    "smk_vos_score", "smk_vos_score_dev", "smk_host_trk_plan", "smk_host_trk_advance",
    "smk_vos_score_ex", "smk_vos_score_dev_ex", "smk_label_rects", "smk_frame_sums", "smk_trk_start", "smk_crop_exemplar_dev",
    "smk_host_trk_start", "smk_vot_overlap", "smk_host_vot_overlap",
    "smk_crop_resize_dev_v", "smk_crop_exemplar_dev_v", "smk_frame_sums_v", "smk_trk_start_v", "smk_host_trk_start_v",
    "smk_paste_mask_dev_v", "smk_vot_overlap_dev",
    "smk_set_stream_hp", "smk_trk_advance_hp", "smk_host_trk_advance_hp",
    "smk_iou_score", "smk_iou_score_dev",
    "smk_mask_rbox_workspace_ex", "smk_mask_rbox_ex", "smk_test_mask_rbox_paths",
    "smk_rle_workspace", "smk_rle_encode", "smk_paste_rle_dev", "smk_test_rle_encode",
    "smk_paste_rle_dev_v", "smk_rle_encode_v", "smk_test_rle_encode_v",
    "smk_labels_rle_encode", "smk_vos_rle", "smk_vos_rle_dev",
    "smk_vos_rle_v", "smk_vos_rle_dev_v", "smk_vos_score_v", "smk_vos_score_dev_v",
    "smk_png_worst_bytes", "smk_png_workspace", "smk_png_encode", "smk_host_png_encode", "smk_vos_png_v", "smk_vos_png_dev_v",
    "smk_vot_traj_overlap", "smk_eao_workspace_bytes", "smk_eao_curve",
    "smk_host_vot_quantise", "smk_host_vot_traj_overlap", "smk_host_eao_curve",
    "smk_ope_curve", "smk_host_ope_curve",
    "smk_vot_step_rows_dev", "smk_host_vot_step_rows",
    "smk_jpeg_tables_bytes", "smk_host_jpeg_parse", "smk_jpeg_workspace", "smk_jpeg_decode", "smk_host_jpeg_decode", "smk_test_jpeg_stages",
)


class ConvGeom(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in (
        "B", "Cin", "H", "W", "Cout", "k", "stride", "pad", "dil", "relu", "res_mode",
        "win", "ups", "Hl", "Wl", "org_y", "org_x", "pos_mul", "pos_add", "cin_off", "cin_len")]


class SeqOp(ctypes.Structure):
    """smk_seq_op: one layer of an smk_op_conv_seq sequence"""
    _fields_ = [("g", ConvGeom), ("src", ctypes.c_int), ("res_src", ctypes.c_int), ("sync", ctypes.c_int),
                ("cfg", ctypes.c_int), ("kstag", ctypes.c_int), ("w_host", ctypes.c_void_p), ("b_host", ctypes.c_void_p),
                ("y_dev", ctypes.c_void_p)]


class TrkCfg(ctypes.Structure):
    """smk_trk_cfg: the tracker's configuration for the scalar kernels (utils/tracker_config.py + hp)"""
    _fields_ = [("context_amount", ctypes.c_double), ("lr", ctypes.c_double)] + [(n, ctypes.c_int) for n in (
        "exemplar_size", "instance_size", "total_stride", "base_size", "score_size", "mask_size")]


class ImageRef(ctypes.Structure):
    """smk_image_ref: the frame of one stream (device pointer, bytes between rows, width, height)"""
    _fields_ = [("data", ctypes.c_void_p), ("row_bytes", ctypes.c_int64), ("w", ctypes.c_int32), ("h", ctypes.c_int32)]


class SmkError(RuntimeError):
    code = 0      # the library's SMK_E_* return code (0: raised on the Python side)


E_SEQ = -6        # SMK_E_SEQ: the persistent sequence kernel reported a failure; the frame is to be re-submitted


def build_library(force=False, verbose=False):
    """Compile the HIP sources for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean"], stdout=subprocess.DEVNULL)
    out = subprocess.run(["make", "-C", CSRC, "-j", "4"], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, universal_newlines=True)
    if verbose or out.returncode != 0:
        print(out.stdout)
    if out.returncode != 0:
        raise SmkError("building libsiammask_hip.so failed")
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SmkError(
            "%s is missing: the HIP extension has not been built (run `python -c 'import "
            "__graft_entry__ as g; g.build()'` or `make -C siammask_amd/csrc`). There is no "
            "CPU fallback." % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    vp, ci, fp = ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p
    L.smk_version.restype = ci
    L.smk_last_error.restype = ctypes.c_char_p
    L.smk_create.argtypes = [ctypes.POINTER(vp), ci, ci, ci, ci]
    L.smk_destroy.argtypes = [vp]
    L.smk_set_weight.argtypes = [vp, ctypes.c_char_p, fp, ctypes.POINTER(ctypes.c_int64), ci]
    L.smk_finalize_weights.argtypes = [vp]
    L.smk_template.argtypes = [vp, fp, ci, vp]
    L.smk_track.argtypes = [vp, fp, ci, ci, fp, fp, fp, vp]
    L.smk_refine.argtypes = [vp, vp, ci, ci, fp, vp]
    L.smk_set_decode_params.argtypes = [vp, fp, ci, ci, ctypes.c_double, ctypes.c_double]
    L.smk_decode.argtypes = [vp, fp, fp, ci, fp, vp, fp, vp]
    L.smk_step.argtypes = [vp, fp, ci, ci, fp, fp, fp, fp, fp, fp, vp]
    L.smk_set_graph_mode.argtypes = [vp, ci]
    L.smk_debug_seq_inject.argtypes = [vp, ci]
    L.smk_set_result_ring.argtypes = [vp, vp, vp, ci, ci]
    L.smk_set_pipeline.argtypes = [vp, ci]
    L.smk_pipeline_join.argtypes = [vp, vp]
    L.smk_pipeline_observe.argtypes = [vp, vp]
    L.smk_result_ring_cursor.argtypes = [vp, ctypes.POINTER(ci), ci, vp]
    L.smk_seq_sync_check.argtypes = [vp, vp, ctypes.POINTER(ci)]
    L.smk_tune.argtypes = [ctypes.c_char_p, ci]
    L.smk_tune_get.argtypes = [ctypes.c_char_p, ctypes.POINTER(ci)]
    L.smk_profile.argtypes = [vp, ci]
    L.smk_profile_dump.argtypes = [vp, ctypes.c_char_p, ci]
    ip = ctypes.POINTER(ci)
    L.smk_debug_read.argtypes = [vp, ctypes.c_char_p, fp, ip, ip, ip, vp]
    gp = ctypes.POINTER(ConvGeom)
    L.smk_op_conv2d_ex.argtypes = [ci, ci, gp, fp, fp, fp, fp, vp, fp, vp]
    L.smk_op_conv2d.argtypes = [ci, ci, fp, ci, ci, ci, ci, fp, fp, ci, ci, ci, ci, ci, ci, fp, fp, vp]
    L.smk_op_dw_xcorr.argtypes = [ci, fp, fp, ci, ci, ci, ci, ci, ci, fp, vp]
    L.smk_op_maxpool3x3s2.argtypes = [ci, fp, ci, ci, ci, ci, fp, vp]
    L.smk_op_stem_pool.argtypes = [fp, fp, fp, ci, ci, fp, fp, vp]
    L.smk_op_l1_block.argtypes = [fp] * 9 + [ci, ci, ci, fp, vp]
    L.smk_host_conv2d_ex.argtypes = [gp, fp, fp, fp, fp, vp, fp]
    L.smk_host_plan_conv.argtypes = [gp, ci, ci, ip, ip, ip, ip]
    L.smk_host_arena_elems.argtypes = [ci, ci, ci, ctypes.POINTER(ctypes.c_uint64)]
    L.smk_host_chain_rows.argtypes = [ci, ci, ip]
    L.smk_packed_size.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    L.smk_export_packed.argtypes = [vp, vp, ctypes.c_uint64]
    L.smk_import_packed.argtypes = [vp, vp, ctypes.c_uint64]
    L.smk_crop_resize.argtypes = [vp, ctypes.c_int64, ci, ci, vp, vp, ci, ci, fp, vp]
    L.smk_paste_mask.argtypes = [fp, ci, vp, ci, ci, ci, ctypes.c_float, ctypes.c_float, vp, fp, vp]
    L.smk_paste_labels.argtypes = [fp, ci, vp, ci, ci, ci, ctypes.c_float, ctypes.c_float, vp, vp]
    L.smk_mask_rbox_workspace.argtypes = [ci, ci, ci]
    L.smk_mask_rbox.argtypes = [vp, ci, ci, ci, ctypes.c_double, vp, ctypes.c_size_t, vp, vp]
    L.smk_mask_rbox_workspace_ex.argtypes = [ci, ci, ci, ci]
    L.smk_mask_rbox_ex.argtypes = [vp, ci, ci, ci, ctypes.c_double, ci, vp, ctypes.c_size_t, vp, vp]
    L.smk_test_mask_rbox_paths.argtypes = [vp, ci, ci, ci, ci, vp]
    cp = ctypes.POINTER(TrkCfg)
    L.smk_trk_state_bytes.argtypes = [ci]
    L.smk_trk_set.argtypes = [vp, ci, vp, vp, vp, ci, ci, vp]
    L.smk_trk_plan.argtypes = [vp, ci, cp, vp]
    L.smk_trk_advance.argtypes = [vp, ci, cp, vp, ci, vp, ci, vp]
    L.smk_host_trk_plan.argtypes = [vp, ci, cp]
    L.smk_host_trk_advance.argtypes = [vp, ci, cp, vp, ci, vp, ci]
    L.smk_crop_resize_dev.argtypes = [vp, ctypes.c_int64, ci, ci, vp, ci, ci, fp, vp]
    L.smk_paste_mask_dev.argtypes = [fp, fp, ci, ci, vp, ci, ci, ci, ci, ctypes.c_float, ctypes.c_float, vp, fp, vp]
    cf, u32 = ctypes.c_float, ctypes.c_uint32
    L.smk_vos_score.argtypes = [fp, ci, vp, ci, ci, ci, cf, vp, vp, u32, vp, ci, cf, vp, vp, vp]
    L.smk_vos_score_dev.argtypes = [fp, fp, ci, ci, vp, ci, ci, ci, ci, cf, vp, vp, u32, vp, ci, cf, vp, vp, vp]
    L.smk_vos_score_ex.argtypes = L.smk_vos_score.argtypes[:-1] + [u32, vp, vp]
    L.smk_vos_score_dev_ex.argtypes = L.smk_vos_score_dev.argtypes[:-1] + [u32, vp, vp]
    i64 = ctypes.c_int64
    L.smk_label_rects.argtypes = [vp, ci, ci, vp, ci, vp, vp]
    L.smk_frame_sums.argtypes = [vp, i64, ci, ci, ci, vp, vp]
    L.smk_trk_start.argtypes = [vp, ci, cp, u32, vp, vp, vp, vp, i64, ci, ci, vp, vp, vp]
    L.smk_host_trk_start.argtypes = [vp, ci, cp, u32, vp, vp, vp, vp, i64, ci, ci, vp, vp]
    L.smk_crop_exemplar_dev.argtypes = [vp, i64, ci, ci, vp, vp, vp, u32, ci, ci, fp, vp]
    L.smk_vot_overlap.argtypes = [vp, ci, vp, vp, ci, ci, ci, vp, vp, vp]
    L.smk_host_vot_overlap.argtypes = [vp, vp, ci, ci, ci, vp, vp]
    L.smk_crop_resize_dev_v.argtypes = [vp, vp, ci, ci, fp, vp]
    L.smk_crop_exemplar_dev_v.argtypes = [vp, vp, vp, vp, u32, ci, ci, fp, vp]
    L.smk_frame_sums_v.argtypes = [vp, ci, vp, vp]
    L.smk_trk_start_v.argtypes = [vp, ci, cp, u32, vp, vp, vp, vp, i64, vp, vp, vp, vp]
    L.smk_host_trk_start_v.argtypes = [vp, ci, cp, u32, vp, vp, vp, vp, i64, vp, vp, vp]
    L.smk_paste_mask_dev_v.argtypes = [fp, fp, ci, ci, vp, ci, ci, ci, ci, vp, cf, cf, vp, vp]
    L.smk_vot_overlap_dev.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp, vp]
    L.smk_set_stream_hp.argtypes = [vp, vp]
    L.smk_trk_advance_hp.argtypes = [vp, ci, cp, vp, vp, ci, vp, ci, vp]
    L.smk_host_trk_advance_hp.argtypes = [vp, ci, cp, vp, vp, ci, vp, ci]
    L.smk_iou_score.argtypes = [fp, ci, vp, ci, ci, ci, cf, vp, i64, vp, ci, cf, vp, vp, vp]
    L.smk_iou_score_dev.argtypes = [fp, fp, ci, ci, vp, ci, ci, ci, ci, cf, vp, i64, vp, ci, cf, vp, vp, vp]
    L.smk_rle_workspace.argtypes = [ci, ci, ci]
    L.smk_rle_encode.argtypes = [vp, ci, ci, ci, ci, vp, ctypes.c_size_t, vp, vp, vp]
    L.smk_test_rle_encode.argtypes = [vp, ci, ci, ci, ci, vp, ctypes.c_size_t, vp, vp, ci, vp]
    L.smk_paste_rle_dev.argtypes = [fp, fp, ci, ci, vp, ci, ci, ci, ci, cf, cf, ci, vp, ctypes.c_size_t, vp, vp, vp]
    L.smk_rle_encode_v.argtypes = [vp, ci, ci, ci, vp, u32, ci, vp, ctypes.c_size_t, vp, vp, vp]
    L.smk_test_rle_encode_v.argtypes = [vp, ci, ci, ci, vp, u32, ci, vp, ctypes.c_size_t, vp, vp, ci, vp]
    L.smk_paste_rle_dev_v.argtypes = [fp, fp, ci, ci, vp, ci, ci, ci, ci, vp, u32, cf, cf, ci, vp, ctypes.c_size_t, vp, vp, vp]
    L.smk_labels_rle_encode.argtypes = [vp, ci, ci, ci, ci, vp, ctypes.c_size_t, vp, vp, vp]
    rle_tail = [u32, vp, ci, vp, ctypes.c_size_t, vp, vp, vp]        # given_mask, init labels, cap, workspace, its bytes, outputs, stream
    L.smk_vos_rle.argtypes = [fp, ci, vp, ci, ci, ci, cf, vp, u32, cf] + rle_tail
    L.smk_vos_rle_dev.argtypes = [fp, fp, ci, ci, vp, ci, ci, ci, ci, cf, vp, u32, cf] + rle_tail
    # groups (count, masks, sizes, init label pointers, live mask), border, ids, alive, seg_thr, given, cap, workspace, outputs, stream
    rle_v_tail = [ci, vp, vp, vp, u32, cf, vp, u32, cf, u32, ci, vp, ctypes.c_size_t, vp, vp, vp]
    L.smk_vos_rle_v.argtypes = [fp, ci, vp, ci, ci, ci] + rle_v_tail
    L.smk_vos_rle_dev_v.argtypes = [fp, fp, ci, ci, vp, ci, ci, ci, ci] + rle_v_tail
    L.smk_png_worst_bytes.argtypes = [ci, ci]
    L.smk_png_workspace.argtypes = [ci, ci, ci, ci]
    L.smk_png_encode.argtypes = [vp, ci, ci, ci, ci, vp, ctypes.c_size_t, vp, vp, vp]
    L.smk_host_png_encode.argtypes = [vp, ci, ci, ci, ci, vp, vp]
    L.smk_vos_png_v.argtypes = [fp, ci, vp, ci, ci, ci] + rle_v_tail                 # (cap in bytes; a byte stream in the counts' place)
    L.smk_vos_png_dev_v.argtypes = [fp, fp, ci, ci, vp, ci, ci, ci, ci] + rle_v_tail
    # groups (count, masks, sizes, gt pointers, init label pointers, live mask), border, ids, alive, given, thrs, their number, counts, stream
    score_v_tail = [ci, vp, vp, vp, vp, u32, cf, vp, u32, u32, vp, ci, vp, vp]
    L.smk_vos_score_v.argtypes = [fp, ci, vp, ci, ci, ci] + score_v_tail
    L.smk_vos_score_dev_v.argtypes = [fp, fp, ci, ci, vp, ci, ci, ci, ci] + score_v_tail
    L.smk_vot_traj_overlap.argtypes = [vp] * 8 + [ci] * 5 + [vp, vp, vp]
    L.smk_eao_workspace_bytes.argtypes = [ci, ci]
    L.smk_eao_curve.argtypes = [vp] * 4 + [ci] * 7 + [vp, ctypes.c_size_t, vp, vp, vp, vp]
    L.smk_host_vot_quantise.argtypes = [vp, ci, vp]
    L.smk_host_vot_traj_overlap.argtypes = [vp] * 5 + [ci] * 5 + [vp, vp]
    L.smk_host_eao_curve.argtypes = [vp] * 3 + [ci] * 6 + [vp] * 5 + [ci]
    L.smk_ope_curve.argtypes = [vp] * 4 + [ci] * 3 + [vp, ci, vp, ci, ci] + [vp] * 4
    L.smk_host_ope_curve.argtypes = [vp] * 3 + [ci] * 3 + [vp, ci, vp, ci, ci] + [vp] * 3
    # pred, stride, adv, gt, state | im_wh, B, row, vid, t, live, N, V, skip, vstate, code, poly, overlap, counts, start_out[, stream]
    L.smk_vot_step_rows_dev.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp, vp, u32, ci, ci, ci] + [vp] * 7
    L.smk_host_vot_step_rows.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp, vp, u32, ci, ci, ci] + [vp] * 6
    sz = ctypes.c_size_t
    L.smk_jpeg_tables_bytes.argtypes = []
    L.smk_host_jpeg_parse.argtypes = [vp, sz, vp, vp, sz, vp, sz]
    L.smk_jpeg_workspace.argtypes = [vp, ci]
    L.smk_jpeg_decode.argtypes = [vp, sz, vp, vp, vp, sz, vp, sz, ci, vp, sz, vp, vp]
    L.smk_host_jpeg_decode.argtypes = [vp, sz, vp, i64, ci, ci, vp]
    L.smk_test_jpeg_stages.argtypes = [ci]
    L.smk_op_conv_seq.argtypes = [ctypes.POINTER(SeqOp), ci, fp, ci, ctypes.POINTER(ctypes.c_float), fp, ip, vp]
    L.smk_host_plan_seq.argtypes = [ctypes.POINTER(SeqOp), ci, ci, ip, ip, ip]
    L.smk_bench_conv.argtypes = [ci, ci, gp, ci, ci, ctypes.POINTER(ctypes.c_float), vp]
    for name in SYMBOLS:
        fn = getattr(L, name)
        if name not in ("smk_last_error",):
            fn.restype = ctypes.c_size_t if name in ("smk_mask_rbox_workspace", "smk_mask_rbox_workspace_ex", "smk_trk_state_bytes",
                                                        "smk_rle_workspace", "smk_eao_workspace_bytes", "smk_png_worst_bytes",
                                                        "smk_png_workspace", "smk_jpeg_tables_bytes", "smk_jpeg_workspace") else ci
    _lib = L
    # SMK_TUNE="key=value,key=value": library tuning knobs from the environment (A/B runs of the test-suite)
    for kv in filter(None, os.environ.get("SMK_TUNE", "").split(",")):
        k, v = kv.split("=")
        check(L.smk_tune(k.strip().encode(), int(v)))
    return L


def check(rc):
    if rc != 0:
        msg = lib().smk_last_error()
        e = SmkError("libsiammask_hip error %d: %s" % (rc, msg.decode() if msg else "?"))
        e.code = rc
        raise e


def current_stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def tune(**kw):
    """Set process-wide tuning knobs of the library (A/B measurements)."""
    for k, v in kw.items():
        check(lib().smk_tune(k.encode(), int(v)))


def tune_get(key):
    """Current value of a tuning knob (so that a test can put back what it changed)."""
    v = ctypes.c_int(0)
    check(lib().smk_tune_get(key.encode(), ctypes.byref(v)))
    return v.value
