"""sc2_det_postprocess without a GPU: the header's symbols and caps and their mirror in hip.py, the entry point's argument checks
(made before anything is launched), and the routing of `RoIHeads.postprocess_detections` between the kernel and the loop."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_det_post as RP  # noqa: E402

HEADER = os.path.join(os.path.dirname(HERE), 'include', 'sc2_bottleneck.h')


def header_defines():
    text = open(HEADER).read()
    return text, {m.group(1): int(m.group(2)) for m in re.finditer(r'#define (SC2_DETPOST_\w+) (\d+)', text)}


def test_header_declares_the_entry_and_the_caps(S):
    text, d = header_defines()
    assert re.search(r'\bint sc2_det_postprocess\(const float \*logits', text)
    assert re.search(r'\blong long sc2_det_postprocess_ws_bytes\(int R, int C, int n, int D\);', text)
    # the caps' floors: 19 classes of a row can pass 0.05, times 1 000 proposals; a class holds at most the proposals
    assert d['SC2_DETPOST_MAX_CAND'] >= 19000 and d['SC2_DETPOST_MAX_SEG'] >= 1000
    assert d['SC2_DETPOST_MAX_CLASSES'] == 128 and d['SC2_DETPOST_MAX_DET'] == 1024
    hip = S.hip
    assert (hip.DETPOST_MAX_CAND, hip.DETPOST_MAX_SEG, hip.DETPOST_MAX_CLASSES, hip.DETPOST_MAX_DET, hip.DETPOST_OVER_CAND,
            hip.DETPOST_OVER_SEG) == tuple(d['SC2_DETPOST_' + k] for k in ('MAX_CAND', 'MAX_SEG', 'MAX_CLASSES', 'MAX_DET', 'OVER_CAND',
                                                                          'OVER_SEG'))
    assert 'sc2_det_postprocess' in hip.ABI_SYMBOLS and 'sc2_det_postprocess_ws_bytes' in hip.ABI_SYMBOLS
    assert callable(hip.det_postprocess)


def test_the_switch_exists_and_configures(S):
    hip = S.hip
    assert isinstance(hip.HostPolicy.det_post_hip, bool) and hip.host_policy.det_post_hip == hip.HostPolicy.det_post_hip
    try:
        hip.configure(det_post_hip=not hip.HostPolicy.det_post_hip)
        assert hip.host_policy.det_post_hip != hip.HostPolicy.det_post_hip
    finally:
        hip.configure(det_post_hip=hip.HostPolicy.det_post_hip)


def test_workspace_size_and_ranges(S):
    hip = S.hip
    r16 = lambda v: (v + 15) // 16 * 16      # noqa: E731
    for R, C, n, D in ((6000, 91, 6, 100), (1, 2, 1, 1), (0, 5, 3, 7), (1000, 128, 2, 1024)):
        cand, lists = R * (C - 1), n * (C - 1)
        want = r16(cand * 16) + r16(lists * D * 8) + r16(R * 16) + r16(cand * 4) + 2 * r16(lists * 4)
        assert hip.det_postprocess_ws_bytes(R, C, n, D) == want
    for R, C, n, D in ((10, 1, 1, 10), (10, 129, 1, 10), (10, 5, 1, 0), (10, 5, 1, 1025), (-1, 5, 1, 10), (10, 5, 65536, 10),
                       (2 ** 31 - 1, 3, 1, 10)):
        assert hip.det_postprocess_ws_bytes(R, C, n, D) == 0


def call_raw(S, R, C, n, D, offsets, thresh=0.05):
    """the entry point with NULL device pointers: every refusal below comes before anything is launched"""
    host = (ctypes.c_int32 * len(offsets))(*offsets)
    null = ctypes.c_void_p(0)
    return S.hip.lib().sc2_det_postprocess(null, null, null, null, host, null, R, C, n, 10.0, 10.0, 5.0, 5.0, 4.135, thresh, 0.01, 0.5, D,
                                           null, null, null, null, null, null, null, null, null)


def test_entry_point_refuses_before_launching(S):
    assert call_raw(S, 10, 1, 1, 100, [0, 10]) == -2 and 'classes' in S.hip.last_error()
    assert call_raw(S, 10, 129, 1, 100, [0, 10]) == -2
    assert call_raw(S, 10, 5, 1, 1025, [0, 10]) == -2 and 'detections per image' in S.hip.last_error()
    assert call_raw(S, 10, 5, 1, 0, [0, 10]) == -2
    for bad in ([1, 10], [0, 9], [0, 11], ):
        assert call_raw(S, 10, 5, 1, 100, bad) == -1 and 'offsets' in S.hip.last_error()
    assert call_raw(S, 10, 5, 2, 100, [0, 7, 5]) == -1
    assert call_raw(S, 10, 5, 1, 100, [0, 10], thresh=float('nan')) == -1 and 'NaN' in S.hip.last_error()
    assert call_raw(S, 10, 5, 1, 100, [0, 10]) == -1 and 'null' in S.hip.last_error()      # well-formed, but no buffers
    assert call_raw(S, 0, 5, 0, 100, [0]) == 0                                                # no image: nothing to do


class OnDevice(torch.Tensor):
    """a CPU tensor that says it lives on the device: what routes `postprocess_detections` to the kernel"""
    is_cuda = property(lambda self: True)


def heads_and_inputs(S, D=100):
    from sc2bench_amd import detection
    counts, C, sizes = (40, 0, 25), 5, ((120, 160), (90, 90), (200, 140))
    logits, deltas, props = RP.random_case(counts, C, sizes, seed=1)
    heads = detection.RoIHeads(None, None, None, score_thresh=0.05, nms_thresh=0.5, detections_per_img=D)
    return heads, torch.from_numpy(logits), torch.from_numpy(deltas), list(torch.from_numpy(props).split(list(counts), 0)), list(sizes)


def same_lists(a, b):
    return all(len(x) == len(y) and all(torch.equal(p.as_subclass(torch.Tensor), q.as_subclass(torch.Tensor)) for p, q in zip(x, y))
               for x, y in zip(a, b))


def test_cpu_tensors_take_the_loop(S, monkeypatch):
    heads, logits, deltas, props, sizes = heads_and_inputs(S)

    def never(*a, **k):
        raise AssertionError('the kernel was called for CPU tensors')
    monkeypatch.setattr(S.hip, 'det_postprocess', never)
    assert S.hip.host_policy.nms_hip
    monkeypatch.setattr(S.hip.host_policy, 'det_post_hip', True)
    boxes, scores, labels = heads.postprocess_detections(logits, deltas, props, sizes)
    assert len(boxes) == len(scores) == len(labels) == 3 and labels[1].shape == (0,) and labels[0].shape[0] > 0


def test_routing_on_device_tensors(S, monkeypatch):
    """With tensors that claim the device: the kernel's result is what the module returns while the status words are zero; a
    non-zero status word, the switch off, `nms_hip` off, or `detections_per_img` outside the range give the loop's result."""
    from sc2bench_amd import detection
    heads, logits, deltas, props, sizes = heads_and_inputs(S)
    loop = heads.postprocess_detections(logits, deltas, props, sizes)
    fake = lambda t: t.as_subclass(OnDevice)      # noqa: E731
    calls = []
    state = {'status': [0, 0, 0]}

    def stub(lg, dl, pr, counts, image_sizes, weights, clip, score_thresh, min_size, nms_thresh, D, **kw):
        calls.append((tuple(counts), tuple(image_sizes), tuple(weights), clip, score_thresh, min_size, nms_thresh, D))
        assert lg.shape == (65, 5) and dl.shape == (65, 20) and pr.shape == (65, 4)
        n = len(counts)
        res_counts = [2, 0, 1]
        return S.hip.DetPostResult(torch.arange(n * D * 4, dtype=torch.float32).reshape(n, D, 4), torch.ones(n, D),
                                   torch.full((n, D), 3, dtype=torch.int64),
                                   torch.tensor([res_counts if not any(state['status']) else [0] * n, state['status']], dtype=torch.int32), None)
    monkeypatch.setattr(S.hip, 'det_postprocess', stub)
    # the loop behind the fall-back runs on CPU tensors: its NMS through the torch-op restatement, whatever the tensors claim
    real_nms = detection.batched_nms
    monkeypatch.setattr(S.hip, 'batched_nms', lambda b, s, i, t, tag=None: real_nms(b.as_subclass(torch.Tensor), s.as_subclass(torch.Tensor),
                                                                                   i.as_subclass(torch.Tensor), t))
    monkeypatch.setattr(S.hip.host_policy, 'det_post_hip', True)
    args = (fake(logits), fake(deltas), [fake(p) for p in props], sizes)
    boxes, scores, labels = heads.postprocess_detections(*args)
    assert len(calls) == 1 and calls[0] == ((40, 0, 25), ((120, 160), (90, 90), (200, 140)), (10.0, 10.0, 5.0, 5.0),
                                            detection.BBOX_XFORM_CLIP, 0.05, 1e-2, 0.5, 100)
    assert [b.shape for b in boxes] == [(2, 4), (0, 4), (1, 4)] and [s.shape for s in scores] == [(2,), (0,), (1,)]
    assert labels[0].tolist() == [3, 3] and boxes[2].tolist() == [[800.0, 801.0, 802.0, 803.0]]
    state['status'] = [0, S.hip.DETPOST_OVER_SEG, 0]
    assert same_lists(heads.postprocess_detections(*args), loop) and len(calls) == 2
    state['status'] = [0, 0, 0]
    monkeypatch.setattr(S.hip.host_policy, 'det_post_hip', False)
    assert same_lists(heads.postprocess_detections(*args), loop) and len(calls) == 2
    monkeypatch.setattr(S.hip.host_policy, 'det_post_hip', True)
    monkeypatch.setattr(S.hip.host_policy, 'nms_hip', False)
    assert same_lists(heads.postprocess_detections(*args), loop) and len(calls) == 2
    monkeypatch.setattr(S.hip.host_policy, 'nms_hip', True)
    heads.detections_per_img = S.hip.DETPOST_MAX_DET + 1
    assert same_lists(heads.postprocess_detections(*args), loop) and len(calls) == 2
    heads.detections_per_img = 100
    assert same_lists(heads.postprocess_detections(fake(logits.double()), fake(deltas.double()), [fake(p.double()) for p in props], sizes),
                      heads.postprocess_detections(logits.double(), deltas.double(), [p.double() for p in props], sizes)) and len(calls) == 2
