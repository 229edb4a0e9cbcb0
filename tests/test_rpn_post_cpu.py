"""sc2_rpn_proposals without a GPU: the header's symbols and caps and their mirror in hip.py, the entry point's argument checks
(made before anything is launched), and the routing of `RegionProposalNetwork.forward` between the kernel and `filter_proposals`."""
import ctypes
import os
import re
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_rpn_post as RR  # noqa: E402

HEADER = os.path.join(os.path.dirname(HERE), 'include', 'sc2_bottleneck.h')


def test_header_declares_the_entry_and_the_caps(S):
    text = open(HEADER).read()
    d = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define (SC2_RPNPOST_\w+) (\d+)', text)}
    assert re.search(r'\bint sc2_rpn_proposals\(const float \*const \*objectness', text)
    assert re.search(r'\blong long sc2_rpn_proposals_ws_bytes\(int N, int L, int K, int P\);', text)
    assert d == {'SC2_RPNPOST_MAX_LEVELS': 8, 'SC2_RPNPOST_MAX_PRE_NMS': 2048, 'SC2_RPNPOST_MAX_POST_NMS': 2048,
                 'SC2_RPNPOST_MAX_KEYS': 16384, 'SC2_RPNPOST_MAX_ANCHORS': 2 ** 31 // 4}
    hip = S.hip
    assert (hip.RPNPOST_MAX_LEVELS, hip.RPNPOST_MAX_PRE_NMS, hip.RPNPOST_MAX_POST_NMS, hip.RPNPOST_MAX_KEYS, hip.RPNPOST_MAX_ANCHORS) == \
        tuple(d['SC2_RPNPOST_' + k] for k in ('MAX_LEVELS', 'MAX_PRE_NMS', 'MAX_POST_NMS', 'MAX_KEYS', 'MAX_ANCHORS'))
    assert 'sc2_rpn_proposals' in hip.ABI_SYMBOLS and 'sc2_rpn_proposals_ws_bytes' in hip.ABI_SYMBOLS
    assert callable(hip.rpn_proposals) and callable(hip.rpn_proposals_ws_bytes)
    # training runs K = P = 2 000 and the evaluation shape selects 5 x 1 000: both within the caps
    eval_levels = [(3, 200, 304), (3, 100, 152), (3, 50, 76), (3, 25, 38), (3, 13, 19)]
    assert sum(a * h * w for a, h, w in eval_levels) == 242991
    assert hip.rpn_proposals_in_range(eval_levels, 6, 1000, 1000) and hip.rpn_proposals_in_range(eval_levels, 6, 2000, 2000)


def test_the_switch_exists_and_configures(S):
    hip = S.hip
    assert isinstance(hip.HostPolicy.rpn_post_hip, bool) and hip.host_policy.rpn_post_hip == hip.HostPolicy.rpn_post_hip
    try:
        hip.configure(rpn_post_hip=not hip.HostPolicy.rpn_post_hip)
        assert hip.host_policy.rpn_post_hip != hip.HostPolicy.rpn_post_hip
    finally:
        hip.configure(rpn_post_hip=hip.HostPolicy.rpn_post_hip)


def test_workspace_size_and_ranges(S):
    hip = S.hip
    r16 = lambda v: (v + 15) // 16 * 16      # noqa: E731
    for N, L, K, P in ((6, 5, 1000, 1000), (1, 1, 1, 1), (0, 5, 3, 7), (2, 8, 2048, 2048), (3, 5, 2000, 300), (3, 2, 10, 2000)):
        cand = N * L * K
        want = r16(cand * 16) + r16(N * L * min(K, P) * 8) + 2 * r16(cand * 4) + r16(N * L * 4)
        assert hip.rpn_proposals_ws_bytes(N, L, K, P) == want
    for N, L, K, P in ((1, 0, 10, 10), (1, 9, 10, 10), (1, 5, 0, 10), (1, 5, 2049, 10), (1, 5, 10, 0), (1, 5, 10, 2049), (-1, 5, 10, 10),
                       (65536, 5, 10, 10)):
        assert hip.rpn_proposals_ws_bytes(N, L, K, P) == 0
    assert not hip.rpn_proposals_in_range([(1, 1, 2049)] * 8 + [(1, 1, 1)], 1, 2048, 10)       # nine levels
    assert hip.rpn_proposals_in_range([(1, 1, 2049)] * 8, 1, 2048, 10) and not hip.rpn_proposals_in_range([(1, 1, 2049)] * 7 + [(3, 1, 1)] * 2, 1, 2048, 10)
    assert not hip.rpn_proposals_in_range([(4, 16384, 8192)], 1, 10, 10) and hip.rpn_proposals_in_range([(4, 16384, 8192 - 1)], 1, 10, 10)


def call_raw(S, levels, N=1, K=10, P=10, ptr=0x10000, thresh=0.0, overrides=None):
    """the entry point with pointers that are never read: every refusal below comes before anything is launched.  `ptr`: the
    value of every device pointer; overrides: {argument name: value}"""
    L = len(levels)
    p = dict(obj=ptr, dl=ptr, anchors=ptr, sizes=ptr, boxes=ptr, scores=ptr, count=ptr, ws=ptr)
    p.update(overrides or {})
    vp = ctypes.c_void_p
    n = max(L, 1)
    obj, dl = (vp * n)(*[p['obj']] * n), (vp * n)(*[p['dl']] * n)
    dims = [(ctypes.c_int32 * n)(*([lv[q] for lv in levels] or [1])) for q in range(3)]
    return S.hip.lib().sc2_rpn_proposals(obj, dl, dims[0], dims[1], dims[2], L, vp(p['anchors']), vp(p['sizes']), N, K, P, 0.7, thresh, 1e-3,
                                         1.0, 1.0, 1.0, 1.0, 4.135, vp(p['boxes']), vp(p['scores']), vp(p['count']), vp(0), vp(0), vp(0),
                                         vp(0), vp(p['ws']), vp(0))


def test_entry_point_refuses_before_launching(S):
    lv = [(3, 8, 10), (3, 4, 5)]
    assert call_raw(S, lv, K=0) == -2 and 'pre-NMS' in S.hip.last_error()
    assert call_raw(S, lv, K=2049) == -2
    assert call_raw(S, lv, P=0) == -2 and 'post-NMS' in S.hip.last_error()
    assert call_raw(S, lv, P=2049) == -2
    assert call_raw(S, []) == -2 and 'levels' in S.hip.last_error()
    assert call_raw(S, [(1, 2, 2)] * 9) == -2
    # the key budget: eight levels at K = 2 048 select exactly 16 384 anchors of an image and are taken (no image: nothing is launched)
    assert call_raw(S, [(1, 1, 4096)] * 8, K=2048, P=2048, N=0) == 0 and call_raw(S, [(1, 1, 2048)] * 7 + [(1, 1, 2049)], K=2048, N=0) == 0
    assert call_raw(S, [(4, 16384, 8192)]) == -2 and '2^31' in S.hip.last_error()
    assert call_raw(S, [(3, 0, 10)]) == -1
    assert call_raw(S, lv, N=-1) == -1 and call_raw(S, lv, N=65536) == -1
    assert call_raw(S, lv, thresh=float('nan')) == -1 and 'NaN' in S.hip.last_error()
    assert call_raw(S, lv, ptr=0) == -1 and 'null' in S.hip.last_error()                                 # well-formed, but no buffers
    for name in ('obj', 'dl', 'anchors', 'sizes', 'boxes', 'scores', 'count', 'ws'):                      # bad alignment
        assert call_raw(S, lv, overrides={name: 0x10004}) == -1 and 'aligned' in S.hip.last_error(), name
    assert call_raw(S, lv, N=0) == 0                                                                       # no image: nothing to do


def test_key_budget_follows_from_the_other_caps(S):
    """sum_l min(K, n_l) <= 16 384: with L <= 8 and K <= 2 048 no call within the other caps can pass it (the entry point and
    hip.rpn_proposals_in_range still compute and check the sum: it guards launch 3's LDS should either cap be raised alone)"""
    hip = S.hip
    assert hip.RPNPOST_MAX_LEVELS * hip.RPNPOST_MAX_PRE_NMS == hip.RPNPOST_MAX_KEYS
    assert hip.rpn_proposals_in_range([(1, 1, 5000)] * 8, 1, 2048, 1000)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(hip, 'RPNPOST_MAX_KEYS', 16383)
        assert not hip.rpn_proposals_in_range([(1, 1, 5000)] * 8, 1, 2048, 1000)


class OnDevice(torch.Tensor):
    """a CPU tensor that says it lives on the device: what routes the RPN to the kernel"""
    is_cuda = property(lambda self: True)


class _Computed(torch.nn.Module):
    def __init__(self, out):
        super().__init__()
        self.out = out

    def forward(self, x):
        return self.out


LEVELS = [(3, 8, 10), (3, 4, 5), (3, 2, 3)]
IMAGE = (64, 80)


def rpn_and_inputs(S, wrap=lambda t: t, dtype=torch.float32):
    from sc2bench_amd import detection
    obj, dl, _ = RR.random_case(LEVELS, 2, IMAGE, seed=3, distinct=True)
    head = _Computed(([wrap(torch.from_numpy(o).to(dtype)) for o in obj], [wrap(torch.from_numpy(d).to(dtype)) for d in dl]))
    gen = detection.AnchorGenerator(((16,), (32,), (64,)), ((0.5, 1.0, 2.0),) * 3)
    rpn = detection.RegionProposalNetwork(gen, head, pre_nms_top_n=dict(training=50, testing=50), post_nms_top_n=dict(training=30, testing=30)).eval()
    feats = OrderedDict((str(l), torch.zeros(2, 1, s[1], s[2])) for l, s in enumerate(LEVELS))
    images = detection.ImageList(torch.zeros(2, 3, IMAGE[0], IMAGE[1]), [IMAGE, (60, 70)])
    return rpn, images, feats


def plain(lists):
    return [t.as_subclass(torch.Tensor) for t in lists]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(plain(a), plain(b)))


def test_cpu_tensors_take_the_loop(S, monkeypatch):
    rpn, images, feats = rpn_and_inputs(S)

    def never(*a, **k):
        raise AssertionError('the kernel was called for CPU tensors')
    monkeypatch.setattr(S.hip, 'rpn_proposals', never)
    assert S.hip.host_policy.nms_hip
    monkeypatch.setattr(S.hip.host_policy, 'rpn_post_hip', True)
    with torch.no_grad():
        boxes, losses = rpn(images, feats)
    assert len(boxes) == 2 and losses == {} and all(0 < b.shape[0] <= 30 and b.shape[1] == 4 for b in boxes)


def test_routing_on_device_tensors(S, monkeypatch):
    """With maps that claim the device: the kernel's result is what the module returns; the switch off, `nms_hip` off, another
    dtype, an anchor generator of another class and top-n values or level counts outside the caps give the loop's result"""
    from sc2bench_amd import detection
    fake = lambda t: t.as_subclass(OnDevice)      # noqa: E731
    rpn, images, feats = rpn_and_inputs(S, wrap=fake)
    ref_rpn, _, _ = rpn_and_inputs(S)
    with torch.no_grad():
        loop, _ = ref_rpn(images, feats)
    calls = []

    def stub(obj, dl, anchors, image_sizes, K, P, nms_thresh, score_thresh, min_size, weights, clip, **kw):
        calls.append((tuple(image_sizes), K, P, nms_thresh, score_thresh, min_size, tuple(weights), clip))
        assert [tuple(o.shape) for o in obj] == [(2,) + s for s in LEVELS] and [tuple(d.shape) for d in dl] == [(2, 12) + s[1:] for s in LEVELS]
        assert anchors.shape == (sum(a * h * w for a, h, w in LEVELS), 4)
        return S.hip.RpnPostResult(torch.arange(2 * P * 4, dtype=torch.float32).reshape(2, P, 4), torch.ones(2, P),
                                   torch.tensor([2, 0], dtype=torch.int32), None)
    monkeypatch.setattr(S.hip, 'rpn_proposals', stub)
    # the loop behind the fall-back runs on CPU tensors: its NMS through the torch-op restatement, whatever the tensors claim
    real_nms = detection.batched_nms
    monkeypatch.setattr(S.hip, 'batched_nms', lambda b, s, i, t, tag=None: real_nms(b.as_subclass(torch.Tensor), s.as_subclass(torch.Tensor),
                                                                                   i.as_subclass(torch.Tensor), t))
    monkeypatch.setattr(S.hip.host_policy, 'rpn_post_hip', True)
    with torch.no_grad():
        boxes, _ = rpn(images, feats)
        assert len(calls) == 1 and calls[0] == ((IMAGE, (60, 70)), 50, 30, 0.7, 0.0, 1e-3, (1.0, 1.0, 1.0, 1.0), detection.BBOX_XFORM_CLIP)
        assert [tuple(b.shape) for b in boxes] == [(2, 4), (0, 4)] and boxes[0].tolist() == [[0, 1, 2, 3], [4, 5, 6, 7]]
        monkeypatch.setattr(S.hip.host_policy, 'rpn_post_hip', False)
        assert same(rpn(images, feats)[0], loop) and len(calls) == 1
        monkeypatch.setattr(S.hip.host_policy, 'rpn_post_hip', True)
        monkeypatch.setattr(S.hip.host_policy, 'nms_hip', False)
        assert same(rpn(images, feats)[0], loop) and len(calls) == 1
        monkeypatch.setattr(S.hip.host_policy, 'nms_hip', True)

        class OtherAnchors(detection.AnchorGenerator):
            pass
        mine = rpn.anchor_generator
        rpn.anchor_generator = OtherAnchors(mine.sizes, mine.aspect_ratios)
        assert same(rpn(images, feats)[0], loop) and len(calls) == 1
        rpn.anchor_generator = mine
        for name, value in (('_pre_nms_top_n', S.hip.RPNPOST_MAX_PRE_NMS + 1), ('_post_nms_top_n', S.hip.RPNPOST_MAX_POST_NMS + 1)):
            kept = getattr(rpn, name)
            setattr(rpn, name, dict(training=value, testing=value))
            setattr(ref_rpn, name, dict(training=value, testing=value))
            assert same(rpn(images, feats)[0], ref_rpn(images, feats)[0]) and len(calls) == 1
            setattr(rpn, name, kept)
            setattr(ref_rpn, name, kept)
        rpn64, _, _ = rpn_and_inputs(S, wrap=fake, dtype=torch.float64)
        ref64, _, _ = rpn_and_inputs(S, dtype=torch.float64)
        assert same(rpn64(images, feats)[0], ref64(images, feats)[0]) and len(calls) == 1
        assert len(rpn(images, feats)[0]) == 2 and len(calls) == 2


def test_training_mode_still_concatenates_for_the_loss(S, monkeypatch):
    """in training mode the kernel supplies the proposals and the loss reads the concatenation: the same losses as the loop's"""
    from sc2bench_amd import detection
    fake = lambda t: t.as_subclass(OnDevice)      # noqa: E731
    rpn, images, feats = rpn_and_inputs(S, wrap=fake)
    ref_rpn, _, _ = rpn_and_inputs(S)
    targets = [dict(boxes=torch.tensor([[5.0, 8.0, 40.0, 50.0]])), dict(boxes=torch.tensor([[10.0, 10.0, 30.0, 44.0], [30.0, 5.0, 60.0, 40.0]]))]
    calls = []

    def stub(obj, dl, anchors, image_sizes, K, P, *a, **kw):
        calls.append((K, P))
        return S.hip.RpnPostResult(torch.zeros(2, P, 4), torch.zeros(2, P), torch.tensor([1, 1], dtype=torch.int32), None)
    monkeypatch.setattr(S.hip, 'rpn_proposals', stub)
    monkeypatch.setattr(S.hip.host_policy, 'rpn_post_hip', True)
    monkeypatch.setattr(S.hip.host_policy, 'box_match_hip', False)
    out = []
    for m in (rpn, ref_rpn):
        detection.enable_training(m).train()
        torch.manual_seed(1)
        out.append(m(images, feats, targets))
    assert calls == [(50, 30)] and [tuple(b.shape) for b in out[0][0]] == [(1, 4), (1, 4)]
    assert sorted(out[0][1]) == ['loss_objectness', 'loss_rpn_box_reg']
    for name in out[0][1]:
        assert torch.equal(out[0][1][name].as_subclass(torch.Tensor), out[1][1][name]), name
