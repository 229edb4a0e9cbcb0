"""GPU: sc2_det_postprocess (csrc/det_post.hip) against tests/ref_det_post.py -- stage A within derived bounds of the float64
reference, stage B exactly the f32 reference on the kernel's own candidate table --, `RoIHeads.postprocess_detections` on the kernel
against the loop of torch ops, and the whole Faster R-CNN once.

THE BOUNDS OF STAGE A.  u = 2^-24 (one f32 rounding, relative); the device `expf` is documented to 1 ULP = 2 u.

Score p_c = exp(x_c) / s, x_c = l_c - max, s the sum of the C exponentials.  One subtraction: x_c carries u |x_c|, which the
exponential turns into a relative u |x_c|; the exponential itself 2 u.  The sum: its terms are positive, so their errors weigh in by
their shares, sum_c p_c (|x_c| + 2) u <= (ln C + 2) u because |x_c| <= -ln p_c and the entropy is at most ln C; the tree adds one
rounding per level, 7 levels (classes c and c + 64, then six butterfly steps): 7 u.  One division: u.  Together, relative,
(|x_c| + 2) + (ln C + 2 + 7) + 1 = |x_c| + ln C + 12 units, and absolutely, with p_c |x_c| <= 1 / e,
    |err p_c| <= (1 / e + p_c (ln C + 12)) u,
asserted with 1 % of slack for the second-order terms and 2^-126 for results below the normal range.

Box corner, e.g. x1' = clip(pcx - half_w): widths = x2 - x1 carries u |w|; ctr = x1 + 0.5 w carries 0.5 u |w| + u |ctr|; the weight
division u |dx|; dx * w then 3 u |dx w|; pcx = dx * w + ctr: 3 u |dx w| + 0.5 u |w| + u |ctr| + u |pcx|.  dw = d / ww carries u |dw|
(the cut at bbox_xform_clip does not enlarge it), exp(dw) relative (|dw| + 2) u, times w: + 2 u, times 0.5 exact: half_w carries
(|dw| + 4) u |half_w|.  The corner add / subtract adds u |corner|, the clip to the image enlarges nothing:
    |err corner| <= (3 |dx w| + 0.5 |w| + |ctr| + |pcx| + (|dw| + 4) |half| + |corner|) u,
evaluated in float64 per corner, again with 1 % of slack.  The observed maxima (as fractions of the bounds) are printed.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_det_post as RP  # noqa: E402
import ref_detection as RD  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
U = 2.0 ** -24
WEIGHTS = (10.0, 10.0, 5.0, 5.0)
CLIP = math.log(1000.0 / 16)
GUARD = 256            # sentinel elements on either side of every output and of the workspace
SENTINEL = -7777


def box_bounds(deltas, props, counts, image_sizes):
    """the docstring's bound per corner, float64 [R,C-1,4] (the unclipped corner's magnitude is used: at least the clipped one's)"""
    R = props.shape[0]
    d = np.asarray(deltas, dtype=np.float64).reshape(R, -1, 4)[:, 1:]
    p = np.asarray(props, dtype=np.float64)
    out = np.zeros(d.shape)
    for axis, (wgt_c, wgt_s) in enumerate(((WEIGHTS[0], WEIGHTS[2]), (WEIGHTS[1], WEIGHTS[3]))):
        w = (p[:, 2 + axis] - p[:, axis])[:, None]
        ctr = p[:, axis:axis + 1] + 0.5 * w
        dc = d[:, :, axis] / wgt_c
        ds = np.minimum(d[:, :, 2 + axis] / wgt_s, float(F32(CLIP)))
        pc = dc * w + ctr
        half = 0.5 * np.exp(ds) * w
        common = 3 * np.abs(dc * w) + 0.5 * np.abs(w) + np.abs(ctr) + np.abs(pc) + (np.abs(ds) + 4) * np.abs(half)
        out[:, :, axis] = (common + np.abs(pc - half)) * U * 1.01
        out[:, :, 2 + axis] = (common + np.abs(pc + half)) * U * 1.01
    return out


def arena(shape, dtype, dev):
    """a sentinel-filled buffer with the tensor of `shape` in its middle -> (whole buffer, the view)"""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=dev)
    return whole, whole[GUARD:GUARD + n].view(shape)


def run_kernel(S, dev, case, want_candidates=True):
    """one call with outputs and workspace inside sentinel arenas -> numpy results; the guards are checked here"""
    logits, deltas, props, counts, sizes, D, thresh, min_size, nms = case
    R, C, n = logits.shape[0], logits.shape[1], len(counts)
    arenas = [arena((n, D, 4), torch.float32, dev), arena((n, D), torch.float32, dev), arena((n, D), torch.int64, dev),
              arena((2, n), torch.int32, dev)]
    ws_bytes = S.hip.det_postprocess_ws_bytes(R, C, n, D)
    assert ws_bytes > 0
    ws_whole = torch.full((ws_bytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    res = S.hip.det_postprocess(torch.from_numpy(logits).to(dev), torch.from_numpy(deltas).to(dev), torch.from_numpy(props).to(dev),
                                list(counts), list(sizes), WEIGHTS, CLIP, thresh, min_size, nms, D, out=tuple(v for _, v in arenas),
                                ws=ws_whole[GUARD:GUARD + ws_bytes], want_candidates=want_candidates)
    torch.cuda.synchronize()
    for (whole, view), name in zip(arenas, ('boxes', 'scores', 'labels', 'count_status')):
        host = whole.cpu().numpy()
        assert np.all(host[:GUARD] == SENTINEL) and np.all(host[-GUARD:] == SENTINEL), 'written outside ' + name
        assert not np.any(host[GUARD:-GUARD] == SENTINEL), 'an element of {} was left unwritten'.format(name)
    host = ws_whole.cpu().numpy()
    assert np.all(host[:GUARD] == 0xA5) and np.all(host[-GUARD:] == 0xA5), 'written outside the workspace'
    cand = tuple(t.cpu().numpy() for t in res.candidates) if want_candidates else None
    cs = res.count_status.cpu().numpy()
    return res.boxes.cpu().numpy(), res.scores.cpu().numpy(), res.labels.cpu().numpy(), cs[0], cs[1], cand


def check_case(S, dev, case, name):
    logits, deltas, props, counts, sizes, D, thresh, min_size, nms = case
    C = logits.shape[1]
    boxes, scores, labels, count, status, (cs, cb) = run_kernel(S, dev, case)
    # stage A against float64
    ref_s, ref_b = RP.stage_a_ref(logits, deltas, props, counts, sizes, WEIGHTS, CLIP)
    assert cs.shape == ref_s.shape and cb.shape == ref_b.shape
    assert np.array_equal(np.isnan(cs), np.isnan(ref_s)) and np.array_equal(np.isnan(cb), np.isnan(ref_b)), name + ': NaN pattern'
    ok = ~np.isnan(ref_s)
    s_bound = (1.0 / math.e + ref_s * (math.log(C) + 12.0)) * U * 1.01 + 2.0 ** -126
    s_frac = (np.abs(cs.astype(np.float64) - ref_s)[ok] / s_bound[ok]).max() if ok.any() else 0.0
    okb = np.isfinite(ref_b)
    b_bound = box_bounds(deltas, props, counts, sizes)
    with np.errstate(invalid='ignore'):
        b_frac = (np.abs(cb.astype(np.float64) - ref_b)[okb] / np.maximum(b_bound[okb], 1e-300)).max() if okb.any() else 0.0
    print('det_post stage A {}: max score error {:.3f} of its bound, max corner error {:.3f} of its bound'.format(name, s_frac, b_frac))
    assert s_frac <= 1.0, name + ': a score misses its bound'
    assert b_frac <= 1.0, name + ': a box corner misses its bound'
    # stage B: exactly the sequential f32 reference on the kernel's own table
    want = RP.stage_b_ref(cs, cb, counts, thresh, min_size, nms, D)
    assert status.tolist() == [0] * len(counts), name
    assert count.tolist() == [w[2].shape[0] for w in want], name + ': counts'
    for i, (wb, wsc, wl) in enumerate(want):
        k = wl.shape[0]
        assert labels[i, :k].tolist() == wl.tolist(), '{}: labels of image {}'.format(name, i)
        assert np.array_equal(scores[i, :k], wsc) and np.array_equal(boxes[i, :k], wb), '{}: image {}'.format(name, i)
        assert not boxes[i, k:].any() and not scores[i, k:].any() and not labels[i, k:].any(), '{}: slots behind the count'.format(name)
    return count, want


def make_case(counts, C, sizes, D, seed, thresh=0.05, min_size=0.01, nms=0.5, **kw):
    logits, deltas, props = RP.random_case(counts, C, sizes, seed, **kw)
    return [logits, deltas, props, tuple(counts), tuple(sizes), D, thresh, min_size, nms]


SHAPES = [('c2-r1', (1,), 2, ((64, 64),), 3, {}),
          ('c2-r1000-d100', (1000,), 2, ((300, 400),), 100, dict(logit_scale=2.0, clusters=200)),
          ('c5-63-0-65', (63, 0, 65), 5, ((120, 160), (90, 90), (200, 140)), 100, {}),
          ('c5-64-65-1-d3', (64, 65, 1), 5, ((120, 160), (100, 100), (64, 64)), 3, {}),
          ('c91-r1000', (1000,), 91, ((400, 600),), 100, dict(logit_scale=3.0, clusters=60)),
          ('c91-1-64-63-d100', (1, 64, 63), 91, ((64, 64), (200, 300), (150, 150)), 100, dict(logit_scale=5.0))]


@pytest.mark.parametrize('shape', SHAPES, ids=[s[0] for s in SHAPES])
def test_random_shapes(S, dev, shape):
    """C in {2, 5, 91}, R_i in {0, 1, 63, 64, 65, 1 000}, n in {1, 3} with unequal images, an image without proposals and (second image of the
    d3 case: its background logit towers) one where nothing passes the score threshold; D = 3 and D = 100 with more kept than D"""
    name, counts, C, sizes, D, kw = shape
    case = make_case(counts, C, sizes, D, seed=len(name) + C, **kw)
    if name == 'c5-64-65-1-d3':
        case[0][64:129, 0] += 40.0
    count, want = check_case(S, dev, case, name)
    if name == 'c5-64-65-1-d3':
        assert count[0] == 3 and count[1] == 0
    if name in ('c2-r1000-d100', 'c91-r1000'):
        assert count[0] == D      # (more than D were kept: the reference without the cut says so)
        full = RP.stage_b_ref(*run_kernel(S, dev, case)[5], counts, case[6], case[7], case[8], 10 ** 6)
        assert full[0][2].shape[0] > D
    if name == 'c5-63-0-65':
        assert count[1] == 0 and count[0] > 0 and count[2] > 0


def test_duplicated_rows_tie_and_suppress_each_other(S, dev):
    """every proposal row twice (rows r and r + 40 are equal in logits, deltas and box): exact score ties, decided by the flat
    index, and the copy falls to its original"""
    case = make_case((80,), 5, ((120, 160),), 100, seed=11)
    for a in case[:3]:
        a[40:] = a[:40]
    count, want = check_case(S, dev, case, 'duplicates')
    half = make_case((80,), 5, ((120, 160),), 100, seed=11)
    half = [a[:40].copy() for a in half[:3]] + [(40,)] + half[4:]
    count_half, want_half = check_case(S, dev, half, 'duplicates-half')
    assert count.tolist() == count_half.tolist() and np.array_equal(want[0][0], want_half[0][0])
    # equal logits only: rows r and r + 40 tie in every class with DIFFERENT boxes, so the flat index shows in the output -- in the
    # order of the tied detections and in which of two overlapping ones stays
    ties = make_case((80,), 5, ((120, 160),), 100, seed=11)
    ties[0][40:] = ties[0][:40]
    count_ties, want_ties = check_case(S, dev, ties, 'ties')
    sc = want_ties[0][1]
    assert (sc[1:] == sc[:-1]).sum() >= 5      # tied neighbours with different boxes made it to the output


def test_chain_across_the_64_boundary(S, dev):
    """ref_detection.chain_case as proposals with zero deltas (the decoded box IS the proposal: small integers) and logits that
    fall with the row: positions 62 .. 65 of the one class are A, B, B, C -- A suppresses both B, which therefore leave C alone"""
    boxes, _, _ = RD.chain_case(0.5)
    n = boxes.shape[0]
    logits = np.stack([np.zeros(n), np.linspace(3.0, -2.0, n)], axis=1).astype(F32)
    case = [logits, np.zeros((n, 8), dtype=F32), boxes.astype(F32), (n,), ((100, 20000),), 200, 0.05, 0.01, 0.5]
    count, want = check_case(S, dev, case, 'chain')
    assert count[0] == n - 2
    x1 = want[0][0][:, 0].tolist()
    assert 6200.0 in x1 and 6204.0 in x1 and 6202.0 not in x1


def test_iou_exactly_on_the_threshold_is_kept(S, dev):
    """[0,0,2,2] over [0,0,2,1] and 10 x 10 over 7 x 10 (zero deltas: the boxes are the proposals, every product exact): IoU
    exactly 1/2 and 7/10 -- not above the threshold, so the second box of each pair stays; a hair below the threshold it goes"""
    props = np.array([[0, 0, 2, 2], [0, 0, 2, 1], [50, 50, 60, 60], [50, 50, 57, 60]], dtype=F32)
    logits = np.stack([np.zeros(4), np.linspace(2.0, 0.0, 4)], axis=1).astype(F32)
    for thr, pair in ((0.5, 0), (0.7, 2)):
        case = [logits, np.zeros((4, 8), dtype=F32), props, (4,), ((100, 100),), 100, 0.05, 0.01, thr]
        count, want = check_case(S, dev, case, 'iou-at-{}'.format(thr))
        kept = want[0][0].tolist()
        assert props[pair].tolist() in kept and props[pair + 1].tolist() in kept
        case[8] = float(np.nextafter(F32(thr), F32(0)))
        count_below, want_below = check_case(S, dev, case, 'iou-below-{}'.format(thr))
        assert props[pair + 1].tolist() not in want_below[0][0].tolist()


def test_clip_value_empty_boxes_and_non_finite_rows(S, dev):
    """dw at, just below, just above and far above bbox_xform_clip; proposals outside the image (clipped to nothing: no candidate);
    rows with a NaN, a +infinite (all scores NaN: no candidate) and a -infinite logit (that class scores 0, the others live)"""
    case = make_case((65,), 5, ((120, 160),), 100, seed=5)
    logits, deltas, props = case[:3]
    for r, f in zip((3, 4, 5, 6), (1.0, 1.0 - 1e-3, 1.0 + 1e-3, 30.0)):
        deltas[r, 2::4] = F32(WEIGHTS[2] * CLIP * f)
        deltas[r, 3::4] = F32(WEIGHTS[3] * CLIP * f)
    props[10] = [400, 10, 430, 40]
    props[11] = [-90, -80, -10, -20]
    deltas[10:12] *= 0.05
    logits[20, 2] = np.nan
    logits[21, 0] = np.inf
    logits[22, 3] = -np.inf
    logits[23, :] = -np.inf
    check_case(S, dev, case, 'specials')
    _, _, _, _, _, (cs, cb) = run_kernel(S, dev, case)
    alive = RP.survivors(cs, cb, 0.05, 0.01)
    assert not alive[[10, 11, 20, 21, 23]].any() and np.isnan(cs[[20, 21, 23]]).all()
    assert cs[22, 2] == 0.0 and np.isfinite(cs[22]).all()
    assert (cb[10, :, 2] - cb[10, :, 0] == 0).all() and (cb[11, :, 3] == 0).all()


def cap_case(C, R, seed=2):
    """score_thresh = 0 and min_size = 0: every candidate survives (scores positive: the logits are narrow)"""
    return make_case((R,), C, ((600, 800),), 100, seed=seed, thresh=0.0, min_size=0.0, logit_scale=1.0, delta_scale=0.5, clusters=40)


def test_exactly_at_the_caps(S, dev):
    """10 classes x 2 048 rows = SC2_DETPOST_MAX_CAND survivors, SC2_DETPOST_MAX_SEG in every class: the kernel path"""
    C, R = 11, S.hip.DETPOST_MAX_SEG
    assert R * (C - 1) == S.hip.DETPOST_MAX_CAND
    case = cap_case(C, R)
    count, want = check_case(S, dev, case, 'at-the-caps')
    assert count[0] == 100


@pytest.mark.parametrize('C,R,bits', [(11, 2049, 3), (2, 20481, 3), (2, 2049, 2)], ids=['c11-r2049', 'c2-one-above', 'c2-segment-only'])
def test_above_a_cap_sets_the_status(S, dev, C, R, bits):
    """one row more than the caps hold (both caps; R (C-1) = MAX_CAND + 1 with one class; the segment cap alone): the status bits,
    count 0, every slot zero -- and an image beside it within the caps keeps its detections"""
    over = cap_case(C, R)
    small = make_case((30,), C, ((600, 800),), 100, seed=4, thresh=0.0, min_size=0.0)
    case = [np.concatenate([a, b]) for a, b in zip(over[:3], small[:3])] + [(R, 30), ((600, 800), (600, 800))] + over[5:]
    boxes, scores, labels, count, status, _ = run_kernel(S, dev, case, want_candidates=False)
    assert status.tolist() == [bits, 0] and count[0] == 0 and count[1] > 0
    assert not boxes[0].any() and not scores[0].any() and not labels[0].any()
    alone = run_kernel(S, dev, small, want_candidates=False)
    assert np.array_equal(alone[0][0], boxes[1]) and np.array_equal(alone[1][0], scores[1]) and np.array_equal(alone[2][0], labels[1])


def test_two_calls_give_the_same_bits(S, dev):
    case = make_case((300, 200), 91, ((300, 400), (200, 200)), 100, seed=9, logit_scale=3.0)
    a, b = run_kernel(S, dev, case), run_kernel(S, dev, case)
    for x, y in zip(a[:5] + a[5], b[:5] + b[5]):
        assert x.tobytes() == y.tobytes()


# ------------------------------------------------------------------------------------------------------------ the module
def module_inputs(dev, counts, C, sizes, seed, **kw):
    logits, deltas, props = RP.random_case(counts, C, sizes, seed, **kw)
    return (torch.from_numpy(logits).to(dev), torch.from_numpy(deltas).to(dev),
            [p.contiguous() for p in torch.from_numpy(props).to(dev).split(list(counts), 0)], list(sizes))


MODULE_CASES = [((40, 0, 25), 5, ((120, 160), (90, 90), (200, 140)), 100, 1), ((64, 30), 7, ((150, 150), (100, 180)), 10, 2)]


@pytest.mark.parametrize('counts,C,sizes,D,seed', MODULE_CASES)
def test_module_on_the_kernel_equals_the_loop(S, dev, monkeypatch, counts, C, sizes, D, seed):
    """`RoIHeads.postprocess_detections` with the switch on against the switch off on the same device tensors: the same counts and
    labels, boxes within 1e-3 px, scores within 1e-5.  Precondition, asserted on the switch-off path's own candidate table: no
    decided IoU within 1e-3 of the threshold, no score within 1e-5 of its threshold or of its neighbour in the order, no side
    within 1e-3 of min_size (the seeds are those of tests/test_det_post_ref_cpu.py)."""
    from sc2bench_amd import detection
    args = module_inputs(dev, counts, C, sizes, seed)
    heads = detection.RoIHeads(None, None, None, score_thresh=0.05, nms_thresh=0.5, detections_per_img=D)
    called = []
    real = S.hip.det_postprocess
    monkeypatch.setattr(S.hip, 'det_postprocess', lambda *a, **k: called.append(1) or real(*a, **k))
    with torch.no_grad():
        monkeypatch.setattr(S.hip.host_policy, 'det_post_hip', False)
        loop = heads.postprocess_detections(*args)
        assert not called
        t_boxes = heads.box_coder.decode(args[1], args[2])
        t_boxes = torch.cat([detection.clip_boxes_to_image(b, hw) for b, hw in zip(t_boxes.split(list(counts), 0), sizes)])
        t_scores = torch.softmax(args[0], -1)
        monkeypatch.setattr(S.hip.host_policy, 'det_post_hip', True)
        got = heads.postprocess_detections(*args)
        assert called == [1]
    m = RP.margins(t_scores[:, 1:].cpu().numpy(), t_boxes[:, 1:].cpu().numpy(), counts, 0.05, 0.01, 0.5)
    assert m['iou'] > 1e-3 and m['score'] > 1e-5 and m['gap'] > 1e-5 and m['side'] > 1e-3, 'seed {}: {}; pick another seed'.format(seed, m)
    assert sum(l.shape[0] for l in loop[2]) > 10
    for i in range(len(counts)):
        assert got[2][i].dtype == torch.int64 and torch.equal(got[2][i], loop[2][i]), 'labels of image {}'.format(i)
        assert got[0][i].shape == loop[0][i].shape and got[0][i].dtype == torch.float32
        if loop[2][i].shape[0]:
            assert (got[0][i] - loop[0][i]).abs().max().item() <= 1e-3 and (got[1][i] - loop[1][i]).abs().max().item() <= 1e-5


def test_module_above_the_cap_returns_the_loops_result(S, dev, monkeypatch):
    """score_thresh = 0 with one row more than the caps hold: the kernel reports it, the module runs the loop -- the same tensors
    as with the switch off"""
    from sc2bench_amd import detection
    args = module_inputs(dev, (2049, 30), 11, ((600, 800), (600, 800)), seed=2, logit_scale=1.0, delta_scale=0.5, clusters=40)
    heads = detection.RoIHeads(None, None, None, score_thresh=0.0, nms_thresh=0.5, detections_per_img=100)
    seen = []
    real = S.hip.det_postprocess

    def spy(*a, **k):
        res = real(*a, **k)
        seen.append(res.count_status.cpu().tolist())
        return res
    monkeypatch.setattr(S.hip, 'det_postprocess', spy)
    with torch.no_grad():
        monkeypatch.setattr(S.hip.host_policy, 'det_post_hip', True)
        got = heads.postprocess_detections(*args)
        monkeypatch.setattr(S.hip.host_policy, 'det_post_hip', False)
        loop = heads.postprocess_detections(*args)
    assert len(seen) == 1 and seen[0][1][0] != 0 and seen[0][1][1] == 0 and seen[0][0][0] == 0
    for g, w in zip(got, loop):
        assert len(g) == len(w) == 2 and all(torch.equal(x, y) for x, y in zip(g, w))
    assert got[2][0].shape[0] == 100


def test_faster_rcnn_end_to_end_on_the_kernel(S, dev, monkeypatch):
    """the full `faster_rcnn_model` once at 320 x 416 with 100 proposals (9 000 candidates at score threshold 0: within the caps):
    the detections come from the kernel and are well formed"""
    from sc2bench_amd import dense
    from test_detection_cpu import BACKBONE_CONFIG, MODEL_KWARGS
    torch.manual_seed(0)
    model = dense.faster_rcnn_model(BACKBONE_CONFIG, min_size=320, max_size=416, box_score_thresh=0.0, rpn_post_nms_top_n_test=100,
                                    **MODEL_KWARGS)
    model.eval().to(dev)
    model.update()
    model.backbone.body.set_compute_dtype('bf16')
    model.backbone.fpn.to(torch.bfloat16)
    x = torch.rand(1, 3, 320, 416, generator=torch.Generator().manual_seed(0)).to(dev)
    seen = []
    real = S.hip.det_postprocess

    def spy(*a, **k):
        res = real(*a, **k)
        seen.append(res.count_status.cpu().tolist())
        return res
    monkeypatch.setattr(S.hip, 'det_postprocess', spy)
    monkeypatch.setattr(S.hip.host_policy, 'det_post_hip', True)
    with torch.no_grad():
        out = model([x[0]])
    torch.cuda.synchronize()
    assert len(seen) == 1 and seen[0][1] == [0]
    boxes, labels, scores = out[0]['boxes'], out[0]['labels'], out[0]['scores']
    d = boxes.shape[0]
    assert d == seen[0][0][0] and 0 < d <= 100 and boxes.shape == (d, 4) and boxes.dtype == torch.float32 and labels.dtype == torch.int64
    assert torch.isfinite(boxes).all() and torch.isfinite(scores).all()
    assert labels.min() >= 1 and labels.max() <= 90 and torch.all(scores[:-1] >= scores[1:])
    assert boxes[:, 0::2].min() >= 0 and boxes[:, 0::2].max() <= 416 and boxes[:, 1::2].min() >= 0 and boxes[:, 1::2].max() <= 320
