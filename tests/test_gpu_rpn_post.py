"""GPU: sc2_rpn_proposals (csrc/rpn_post.hip) against tests/ref_rpn_post.py -- the selection EQUAL to `select_ref`, stage A within
derived bounds of the float64 reference, stage B exactly the f32 reference on the kernel's own candidate table --,
`RegionProposalNetwork.forward` on the kernel against the switch off (evaluation and training), and the whole Faster R-CNN once.

THE BOUNDS OF STAGE A.  u = 2^-24 (one f32 rounding, relative); the device `expf` is documented to 1 ULP = 2 u.

Score s = 1 / (1 + e), e = exp(-x): the negation is exact, the exponential carries 2 u relative; through the sum e's error weighs
e / (1 + e) = 1 - s, so 1 + e carries 2 (1 - s) u from it and u from the add; the division adds u.  Relative, 2 (1 - s) + 2 <= 4 units:
    |err s| <= 4 s u,
asserted with 1 % of slack for the second-order terms and 2^-126 for results below the normal range (a score that leaves it, or an
exponential that overflows to a score of 0, lies within that of the float64 value).

Box corner: tests/test_gpu_det_post.py's bound, derived there for the same operations in the same order (the decode and the clip
are one function of csrc/detect_common.h for both kernels), with the anchor in the proposal's place:
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

import ref_rpn_post as RR  # noqa: E402
import ref_detection as RD  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
U = 2.0 ** -24
WEIGHTS = (1.0, 1.0, 1.0, 1.0)
CLIP = math.log(1000.0 / 16)
GUARD = 256            # sentinel elements on either side of every output and of the workspace
SENTINEL = -7777


def case(obj, dl, anchors, sizes, K, P, nms=0.7, thresh=0.0, min_size=1e-3):
    return dict(obj=obj, dl=dl, anchors=anchors, sizes=tuple(sizes), K=K, P=P, nms=nms, thresh=thresh, min_size=min_size)


def random_case(shapes, sizes, K, P, seed, **kw):
    extra = {k: kw.pop(k) for k in ('nms', 'thresh', 'min_size') if k in kw}
    obj, dl, anchors = RR.random_case(shapes, len(sizes), max(sizes), seed, **kw)
    return case(obj, dl, anchors, sizes, K, P, **extra)


def arena(shape, dtype, dev):
    """a sentinel-filled buffer with the tensor of `shape` in its middle -> (whole buffer, the view)"""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=dev)
    return whole, whole[GUARD:GUARD + n].view(shape)


def run_kernel(S, dev, c, want_candidates=True):
    """one call with outputs and workspace inside sentinel arenas -> numpy (boxes, scores, count, candidates); the guards are checked here"""
    N, L, K, P = len(c['sizes']), len(c['obj']), c['K'], c['P']
    arenas = [arena((N, P, 4), torch.float32, dev), arena((N, P), torch.float32, dev), arena((N,), torch.int32, dev)]
    ws_bytes = S.hip.rpn_proposals_ws_bytes(N, L, K, P)
    assert ws_bytes > 0
    ws_whole = torch.full((ws_bytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    res = S.hip.rpn_proposals([torch.from_numpy(o).to(dev) for o in c['obj']], [torch.from_numpy(d).to(dev) for d in c['dl']],
                              torch.from_numpy(c['anchors']).to(dev), list(c['sizes']), K, P, c['nms'], c['thresh'], c['min_size'], WEIGHTS,
                              CLIP, out=tuple(v for _, v in arenas), ws=ws_whole[GUARD:GUARD + ws_bytes], want_candidates=want_candidates)
    torch.cuda.synchronize()
    for (whole, view), name in zip(arenas, ('boxes', 'scores', 'count')):
        host = whole.cpu().numpy()
        assert np.all(host[:GUARD] == SENTINEL) and np.all(host[-GUARD:] == SENTINEL), 'written outside ' + name
        assert not np.any(host[GUARD:-GUARD] == SENTINEL), 'an element of {} was left unwritten'.format(name)
    host = ws_whole.cpu().numpy()
    assert np.all(host[:GUARD] == 0xA5) and np.all(host[-GUARD:] == 0xA5), 'written outside the workspace'
    cand = tuple(t.cpu().numpy() for t in res.candidates) if want_candidates else None
    return res.boxes.cpu().numpy(), res.scores.cpu().numpy(), res.count.cpu().numpy(), cand


def box_bounds(c, index, k):
    """the docstring's bound per corner, float64 [N,L,K,4] (the unclipped corner's magnitude is used: at least the clipped one's)"""
    N, L, K = index.shape
    out = np.zeros((N, L, K, 4))
    anchors = c['anchors'].astype(np.float64)
    clip = float(F32(CLIP))
    off = 0
    for l in range(L):
        dl = RR.level_deltas(c['dl'][l]).astype(np.float64)
        for i in range(N):
            t = index[i, l, :k[i, l]].astype(np.int64)
            p, d = anchors[off + t], dl[i, t]
            for axis in (0, 1):
                w = p[:, 2 + axis] - p[:, axis]
                ctr = p[:, axis] + 0.5 * w
                dc, ds = d[:, axis], np.minimum(d[:, 2 + axis], clip)
                with np.errstate(invalid='ignore', over='ignore'):
                    pc = dc * w + ctr
                    half = 0.5 * np.exp(ds) * w
                    common = 3 * np.abs(dc * w) + 0.5 * np.abs(w) + np.abs(ctr) + np.abs(pc) + (np.abs(ds) + 4) * np.abs(half)
                    out[i, l, :t.shape[0], axis] = (common + np.abs(pc - half)) * U * 1.01
                    out[i, l, :t.shape[0], 2 + axis] = (common + np.abs(pc + half)) * U * 1.01
        off += dl.shape[1]
    return out


def check_case(S, dev, c, name):
    boxes, scores, count, (ci, cs, cb, ck) = run_kernel(S, dev, c)
    # the selection: equal, place by place
    want_index, want_k = RR.select_batch(c['obj'], c['K'])
    assert np.array_equal(ck, want_k), name + ': k_l'
    assert np.array_equal(ci, want_index), name + ': the selected indices or their order'
    # stage A against float64
    ref_s, ref_b = RR.stage_a_ref(c['obj'], c['dl'], c['anchors'], c['sizes'], want_index, want_k, WEIGHTS, CLIP)
    assert np.array_equal(np.isnan(cs), np.isnan(ref_s)) and np.array_equal(np.isnan(cb), np.isnan(ref_b)), name + ': NaN pattern'
    ok = ~np.isnan(ref_s)
    s_bound = 4.0 * ref_s * U * 1.01 + 2.0 ** -126
    s_frac = (np.abs(cs.astype(np.float64) - ref_s)[ok] / s_bound[ok]).max() if ok.any() else 0.0
    okb = np.isfinite(ref_b)
    with np.errstate(invalid='ignore'):
        b_bound = box_bounds(c, want_index, want_k)
        b_frac = (np.abs(cb.astype(np.float64) - ref_b)[okb] / np.maximum(b_bound[okb], 1e-300)).max() if okb.any() else 0.0
    print('rpn_post stage A {}: max score error {:.3f} of its bound, max corner error {:.3f} of its bound'.format(name, s_frac, b_frac))
    assert s_frac <= 1.0, name + ': a score misses its bound'
    assert b_frac <= 1.0, name + ': a box corner misses its bound'
    # stage B: exactly the sequential f32 reference on the kernel's own table
    want = RR.stage_b_ref(cs, cb, ck, c['thresh'], c['min_size'], c['nms'], c['P'])
    assert count.tolist() == [w[1].shape[0] for w in want], name + ': counts'
    for i, (wb, wsc, _, _) in enumerate(want):
        m = wsc.shape[0]
        assert np.array_equal(scores[i, :m], wsc) and np.array_equal(boxes[i, :m], wb), '{}: image {}'.format(name, i)
        assert not boxes[i, m:].any() and not scores[i, m:].any(), '{}: slots behind the count'.format(name)
    return count, want, (ci, cs, cb, ck)


SIZES3 = ((120, 160), (90, 100), (128, 96))
SHAPES = [
    ('l1-a1-n1-k1-p1', [(1, 1, 1)], ((64, 64),), 1, 1, {}),
    ('l1-a3-k1-p3', [(3, 5, 7)], SIZES3, 1, 3, {}),
    ('l5-a3-k64-p1000', [(3, 8, 10), (3, 4, 5), (3, 2, 3), (3, 1, 2), (3, 1, 1)], SIZES3, 64, 1000, {}),            # n_l = 240, 60, 18, 6, 3
    ('l4-a1-around-k64-p3', [(1, 7, 9), (1, 8, 8), (1, 5, 13), (1, 17, 241)], ((120, 160),), 64, 3, {}),            # n_l = K - 1, K, K + 1, 4 097
    ('l4-around-k1000', [(3, 37, 37), (1, 27, 37), (1, 25, 40), (1, 13, 77)], SIZES3, 1000, 1000, {}),              # n_l = 4 107, 999, 1 000, 1 001
    ('l4-around-k2048', [(1, 23, 89), (1, 32, 64), (1, 3, 683), (3, 2, 683)], ((300, 400),), 2048, 1000, {}),       # n_l = 2 047, 2 048, 2 049, 4 098
]


@pytest.mark.parametrize('shape', SHAPES, ids=[s[0] for s in SHAPES])
def test_random_shapes(S, dev, shape):
    """L in {1, 5}, A in {1, 3}, N in {1, 3} with unequal images, level sizes 1, 60, K - 1, K, K + 1 and 4 097, K in {1, 64, 1 000,
    2 048}, P in {1, 3, 1 000} with more kept than P"""
    name, shapes, sizes, K, P, kw = shape
    c = random_case(shapes, sizes, K, P, seed=len(name) + K, **kw)
    count, want, cand = check_case(S, dev, c, name)
    if name in ('l1-a3-k1-p3', 'l5-a3-k64-p1000'):
        assert len(set(count.tolist())) > 1 or count[0] > 0
    if name == 'l4-a1-around-k64-p3':
        assert count[0] == P      # (more than P were kept: the reference without the cut says so)
        assert RR.stage_b_ref(cand[1], cand[2], cand[3], c['thresh'], c['min_size'], c['nms'], 10 ** 6)[0][1].shape[0] > P
    if name == 'l4-around-k2048':
        assert count[0] == P
        assert RR.stage_b_ref(cand[1], cand[2], cand[3], c['thresh'], c['min_size'], c['nms'], 10 ** 6)[0][1].shape[0] > P


def test_the_largest_real_level(S, dev):
    """one 200 x 304 x 3 level (182 400 anchors, the first level of an 800 x 1216 batch), K = P = 1 000"""
    c = random_case([(3, 200, 304)], ((800, 1216),), 1000, 1000, seed=3)
    count, want, _ = check_case(S, dev, c, 'level-200x304x3')
    assert 0 < count[0] <= 1000


def test_the_key_budget_exactly_at_the_cap(S, dev):
    """eight levels of 2 050 anchors at K = 2 048: 16 384 selected anchors per image, P = 2 048"""
    assert 8 * 2048 == S.hip.RPNPOST_MAX_KEYS
    c = random_case([(1, 41, 50)] * 8, ((200, 240),), 2048, 2048, seed=8)
    count, want, _ = check_case(S, dev, c, 'key-budget')
    assert count[0] > 8


def test_equal_logits_go_by_the_lower_index(S, dev):
    """a level whose logits are all equal: its selection is the first K indices; and 300 copies of one logit straddling the cut of
    another level (more than K - 300 and fewer than K logits above it): the copies of the lowest indices are taken"""
    K = 1000
    c = random_case([(3, 37, 37), (1, 17, 241)], ((200, 240), (180, 200)), K, 1000, seed=4)
    c['obj'][0][:] = F32(0.25)
    rng = np.random.RandomState(0)
    flat = (rng.permutation(4097) / 100.0).astype(F32)                # distinct values 0 .. 40.96
    where = rng.choice(4097, 300, replace=False)
    flat[where] = F32(32.005)
    above = int((flat > F32(32.005)).sum())
    assert above < K < above + 300
    c['obj'][1][0] = flat.reshape(1, 17, 241)
    c['obj'][1][1] = flat[::-1].reshape(1, 17, 241)
    count, want, (ci, cs, cb, ck) = check_case(S, dev, c, 'ties')
    assert ci[0, 0].tolist() == list(range(K)) and ci[1, 0].tolist() == list(range(K))
    assert ci[0, 1, above:].tolist() == sorted(where.tolist())[:K - above]


def test_nan_and_infinite_inputs_and_empty_boxes(S, dev):
    """NaN logits are selected first and dropped at the score test; +inf scores 1, -inf scores 0; -0 and +0 tie; NaN and infinite
    deltas; anchors outside the image are clipped to nothing and dropped"""
    c = random_case([(3, 8, 10), (1, 6, 11)], ((120, 160), (90, 100)), 64, 1000, seed=6)
    o0, o1 = RR.level_logits(c['obj'][0]).copy(), c['obj'][1]
    o0[0, [5, 17, 200]] = np.nan
    o0[0, 30] = np.inf
    o0[0, 31] = -np.inf
    o0[1, 0:240:2] = F32(-0.0)
    o0[1, 1:240:2] = F32(0.0)
    o0[1, 100:110] = F32(-1.0)
    c['obj'][0] = np.ascontiguousarray(o0.reshape(2, 8, 10, 3).transpose(0, 3, 1, 2))
    o1[1, 0, 0, :] = -np.inf
    d0 = c['dl'][0]
    d0[0, 0, 0, 2] = np.nan
    d0[0, 2, 1, 0] = np.nan
    d0[0, 5, 2, 2] = np.inf
    d0[0, 6, 3, 3] = np.inf
    d0[0, 7, 4, 4] = -np.inf
    c['anchors'][240:251] += F32(1000.0)          # the second level's first row: right of every image
    count, want, (ci, cs, cb, ck) = check_case(S, dev, c, 'specials')
    assert sorted(ci[0, 0, :3].tolist()) == [5, 17, 200] and np.isnan(cs[0, 0, :3]).all() and ci[0, 0, 3] == 30 and cs[0, 0, 3] == 1.0
    assert not np.isnan(want[0][1]).any()
    assert ci[1, 0].tolist() == list(range(64))                       # zeros of either sign tie: by index, above the -1s
    alive = RR.survivors(cs, cb, 0.0, 1e-3)
    gone = np.isin(ci[:, 1], np.arange(11)) & (np.arange(64)[None, :] < ck[:, 1:2])
    assert gone.any() and not alive[:, 1][gone].any()
    assert np.isnan(cb).any() and (cs[1, 1][ci[1, 1] < 11] == 0.0).all()


def test_score_threshold_and_an_image_without_survivors(S, dev):
    """score_thresh = 0.5: of the first image about half survive, the second (all logits negative) yields nothing: count 0, zeros"""
    c = random_case([(3, 8, 10), (3, 4, 5)], ((120, 160), (90, 100)), 64, 1000, seed=7, thresh=0.5)
    for o in c['obj']:
        o[1] = -np.abs(o[1]) - F32(0.01)
    o = c['obj'][1]
    o[0].reshape(-1)[:40] = F32(0.0)             # sigmoid(0) = 0.5 exactly: inclusive, these stay
    count, want, (ci, cs, cb, ck) = check_case(S, dev, c, 'threshold')
    assert count[1] == 0 and count[0] > 0
    assert (cs[0, 1] == 0.5).sum() >= 20 and (want[0][1] == 0.5).any()


def test_duplicated_anchors_tie_and_fall_to_their_originals(S, dev):
    """a level twice over (anchor t + n / 2 equals anchor t in logit, deltas and box): exact score ties decided by the rank, and
    the copy falls to its original -- the result is that of the half"""
    half = random_case([(1, 6, 10)], ((120, 160),), 64, 1000, seed=11)
    both = case([np.concatenate([half['obj'][0]] * 2, axis=2)], [np.concatenate([half['dl'][0]] * 2, axis=2)],
                np.concatenate([half['anchors']] * 2), half['sizes'], 128, 1000)
    count, want, (ci, cs, cb, ck) = check_case(S, dev, both, 'duplicates')
    count_half, want_half, _ = check_case(S, dev, half, 'duplicates-half')
    assert (cs[0, 0, 0:120:2] == cs[0, 0, 1:120:2]).all() and (ci[0, 0, 0:120:2] + 60 == ci[0, 0, 1:120:2]).all()
    assert count.tolist() == count_half.tolist() and np.array_equal(want[0][0], want_half[0][0])
    assert (want[0][3] % 2 == 0).all()          # the originals: even ranks


def chain_level(n, at, d):
    """n far-apart 10 x 10 boxes in a row, and at positions at .. at + 3 the chain A, B, B, C of ref_detection.chain_case"""
    boxes = np.zeros((n, 4), dtype=F32)
    for i in range(n):
        boxes[i] = [100.0 * i, 0, 100.0 * i + 10, 10]
    x0 = 100.0 * at
    boxes[at + 1] = boxes[at + 2] = [x0 + d, 0, x0 + d + 10, 10]
    boxes[at + 3] = [x0 + 2 * d, 0, x0 + 2 * d + 10, 10]
    return boxes


def test_chains_across_the_64_and_256_boundaries(S, dev):
    """anchors with zero deltas (the decoded box IS the anchor: small integers) and logits that fall with the index: positions
    62 .. 65 and 254 .. 257 are A, B, B, C -- A suppresses both B, which therefore leave C alone"""
    n = 300
    boxes = chain_level(n, 62, 2.0)
    boxes[254:258] = chain_level(n, 254, 2.0)[254:258]
    logits = np.linspace(3.0, -2.0, n).astype(F32).reshape(1, 1, 1, n)
    c = case([logits], [np.zeros((1, 4, 1, n), dtype=F32)], boxes, ((100, 40000),), 512, 512, nms=0.5)
    count, want, (ci, cs, cb, ck) = check_case(S, dev, c, 'chains')
    assert np.array_equal(cb[0, 0, :n], boxes) and count[0] == n - 4
    x1 = want[0][0][:, 0].tolist()
    for at in (62, 254):
        assert 100.0 * at in x1 and 100.0 * at + 4.0 in x1 and 100.0 * at + 2.0 not in x1


def test_the_cut_at_p_comes_after_the_suppression(S, dev):
    """six 10 x 10 boxes in falling order of their logits, the second over the first (IoU 9 / 11 > 0.7): it is suppressed and takes
    no slot of the P = 3 -- ranks 0, 2 and 3 come out, on one level and on each of two"""
    anchors = np.array([[0, 0, 10, 10], [1, 0, 11, 10], [20, 0, 30, 10], [40, 0, 50, 10], [60, 0, 70, 10], [80, 0, 90, 10]], dtype=F32)
    logits = np.linspace(2.0, 0.0, 6).astype(F32).reshape(1, 1, 1, 6)
    c = case([logits], [np.zeros((1, 4, 1, 6), dtype=F32)], anchors, ((100, 200),), 64, 3)
    count, want, _ = check_case(S, dev, c, 'cut-after-nms')
    assert count[0] == 3 and want[0][3].tolist() == [0, 2, 3] and want[0][0][:, 0].tolist() == [0, 20, 40]
    c = case([logits, logits - F32(0.125)], [np.zeros((1, 4, 1, 6), dtype=F32)] * 2, np.concatenate([anchors, anchors]), ((100, 200),), 64, 5)
    count, want, _ = check_case(S, dev, c, 'cut-after-nms-two-levels')
    assert count[0] == 5 and want[0][2].tolist() == [0, 1, 0, 1, 0] and want[0][3].tolist() == [0, 0, 2, 2, 3]


def test_iou_exactly_on_the_threshold_is_kept(S, dev):
    """[0,0,2,2] over [0,0,2,1] and 10 x 10 over 7 x 10 (zero deltas, every product exact): IoU exactly 1/2 and 7/10 -- not above
    the threshold, so the second box of each pair stays; a hair below the threshold it goes"""
    anchors = np.array([[0, 0, 2, 2], [0, 0, 2, 1], [50, 50, 60, 60], [50, 50, 57, 60]], dtype=F32)
    logits = np.linspace(2.0, 0.0, 4).astype(F32).reshape(1, 1, 1, 4)
    for thr, pair in ((0.5, 0), (0.7, 2)):
        c = case([logits], [np.zeros((1, 4, 1, 4), dtype=F32)], anchors, ((100, 100),), 64, 64, nms=thr)
        count, want, _ = check_case(S, dev, c, 'iou-at-{}'.format(thr))
        kept = want[0][0].tolist()
        assert anchors[pair].tolist() in kept and anchors[pair + 1].tolist() in kept
        c['nms'] = float(np.nextafter(F32(thr), F32(0)))
        count_below, want_below, _ = check_case(S, dev, c, 'iou-below-{}'.format(thr))
        assert anchors[pair + 1].tolist() not in want_below[0][0].tolist()


def test_two_levels_never_suppress_each_other_and_saturated_scores(S, dev):
    """the same anchors, deltas and logits on two levels: every box is kept once per level; logits 17 and 20 both give 1.0f -- of
    the four saturated candidates the lower level goes first, and within a level the greater logit (the lower rank)"""
    one = random_case([(1, 4, 5)], ((120, 160),), 64, 1000, seed=13)
    one['obj'][0].reshape(-1)[[3, 11]] = [F32(17.0), F32(20.0)]
    c = case(one['obj'] * 2, one['dl'] * 2, np.concatenate([one['anchors']] * 2), one['sizes'], 64, 1000)
    count, want, (ci, cs, cb, ck) = check_case(S, dev, c, 'two-levels')
    count_one, want_one, _ = check_case(S, dev, one, 'one-level')
    assert count[0] == 2 * count_one[0]
    assert want[0][1][:4].tolist() == [1.0] * 4 and want[0][2][:4].tolist() == [0, 0, 1, 1] and want[0][3][:4].tolist() == [0, 1, 0, 1]
    assert ci[0, 0, :2].tolist() == [11, 3]


def test_two_calls_give_the_same_bits(S, dev):
    c = random_case([(3, 16, 20), (3, 8, 10), (3, 4, 5)], SIZES3, 300, 200, seed=9)
    a, b = run_kernel(S, dev, c), run_kernel(S, dev, c)
    for x, y in zip(a[:3] + a[3], b[:3] + b[3]):
        assert x.tobytes() == y.tobytes()


# ------------------------------------------------------------------------------------------------------------ the module
class _Computed(torch.nn.Module):
    """stands in for the RPN head: returns what the head computed once (tests/test_gpu_detection.py's idea: the head's
    convolutions are not bit-reproducible from call to call)"""

    def __init__(self, out):
        super().__init__()
        self.out = out

    def forward(self, x):
        return self.out


MODULE_LEVELS = [(3, 40, 52), (3, 20, 26), (3, 10, 13), (3, 5, 7), (3, 3, 4)]      # a 160 x 208 image at strides 4 .. 64
MODULE_IMAGE = (160, 208)


def rpn_and_inputs(dev, seed, top_n, training=False):
    """an RPN whose head returns seeded maps with DISTINCT logits per image (no tie for torch.topk to decide), and its inputs"""
    from collections import OrderedDict
    from sc2bench_amd import detection
    obj, dl, _ = RR.random_case(MODULE_LEVELS, 2, MODULE_IMAGE, seed, logit_scale=4.0, delta_scale=0.2, distinct=True)
    head = _Computed(([torch.from_numpy(o).to(dev).requires_grad_(training) for o in obj],
                      [torch.from_numpy(d).to(dev).requires_grad_(training) for d in dl]))
    gen = detection.AnchorGenerator(((32,), (64,), (128,), (256,), (512,)), ((0.5, 1.0, 2.0),) * 5)
    rpn = detection.RegionProposalNetwork(gen, head, pre_nms_top_n=dict(training=top_n, testing=top_n),
                                          post_nms_top_n=dict(training=top_n, testing=top_n))
    H, W = MODULE_IMAGE
    feats = OrderedDict((str(l), torch.zeros(2, 1, s[1], s[2], device=dev)) for l, s in enumerate(MODULE_LEVELS))
    images = detection.ImageList(torch.zeros(2, 3, H, W, device=dev), [(H, W), (H - 12, W - 20)])
    return rpn, feats, images, obj, dl


def path_slack(c, index, k):
    """how far a corner of the kernel path can lie from the torch-op path's, float64 [N,L,K] (see `assert_margins`)"""
    N, L, K = index.shape
    out = np.zeros((N, L, K))
    anchors = c['anchors'].astype(np.float64)
    clip = float(F32(CLIP))
    off = 0
    for l in range(L):
        dl = RR.level_deltas(c['dl'][l]).astype(np.float64)
        for i in range(N):
            t = index[i, l, :k[i, l]].astype(np.int64)
            p, d = anchors[off + t], dl[i, t]
            for axis in (0, 1):
                w = p[:, 2 + axis] - p[:, axis]
                pc = d[:, axis] * w + (p[:, axis] + 0.5 * w)
                half = 0.5 * np.exp(np.minimum(d[:, 2 + axis], clip)) * w
                slack = (4.1 * np.abs(half) + 2.0 * np.maximum(np.abs(pc - half), np.abs(pc + half))) * U
                out[i, l, :t.shape[0]] = np.maximum(out[i, l, :t.shape[0]], slack)
        off += dl.shape[1]
    return out


def assert_margins(S, dev, rpn, feats, images, obj, dl, top_n, seed):
    """The preconditions of a comparison with the torch-op path, asserted on the float64 table of the reference's own selection.
    Both paths decode a box with the same f32 operations in the same order on the same inputs (`BoxCoder.decode_single` as
    csrc/detect_common.h restates it; torch's ops are separate launches: nothing is contracted), and every one of them but the
    exponential is a correctly rounded IEEE operation: the same bits on both.  The two exponentials (each documented to 1 ULP) differ
    by at most 2 ULP = 4 u relative, so the half sides by 4.1 u |half| (two roundings follow it), and a corner, through the rounding
    of its own add, by at most e = 4.1 u |half| + 2 u |corner| (`path_slack`, per box).  The scores (each within 4 s u of the exact
    value, module docstring) differ by at most 8 u.  No decision may flip within that:
    * adjacent distinct scores of an image's ordered survivors are more than 8 u apart, no score within 8 u of the threshold;
    * no side of a box within 2 e of min_size;
    * for every pair the walk decides (an earlier kept box against a later survivor of its level; e the greater of the two boxes')
      the IoU stays on its side of the threshold for every movement of the eight corners by up to e: with I = w h the intersection,
      |dI| <= 2 e (w + h) + 4 e^2 (each of its sides moves by up to 2 e), the same for each area, and
      (I - dI) / (A + B - I + dA + dB + dI) > thr or (I + dI) / (A + B - I - dA - dB - dI) < thr (or no overlap even after + 2 e)."""
    with torch.no_grad():
        anchors = rpn.anchor_generator(images, list(feats.values()))[0].cpu().numpy()
    index, k = RR.select_batch(obj, top_n)
    s, b = RR.stage_a_ref(obj, dl, anchors, images.image_sizes, index, k, WEIGHTS, CLIP)
    slack = path_slack(dict(dl=dl, anchors=anchors), index, k)
    m = RR.margins(s, b, k, rpn.score_thresh, rpn.min_size, rpn.nms_thresh)
    print('module preconditions, seed {}: largest corner slack {:.2e} px, margins {}'.format(seed, slack.max(), {a: float(v) for a, v in m.items()}))
    assert m['score'] > 8 * U and m['gap'] > 8 * U, 'seed {}: {}; pick another seed'.format(seed, m)
    sides = np.minimum(b[..., 2] - b[..., 0], b[..., 3] - b[..., 1])
    live = np.arange(index.shape[2])[None, None, :] < k[:, :, None]
    assert np.all((np.abs(sides - rpn.min_size) > 2 * slack)[live]), 'seed {}: a side within the slack of min_size; pick another seed'.format(seed)
    thr, pairs = rpn.nms_thresh, 0
    for i in range(s.shape[0]):
        lvl, rank = RR._ordered(s[i].astype(F32), b[i].astype(F32), k[i], rpn.score_thresh, rpn.min_size)
        bb, eb = b[i][lvl, rank], slack[i][lvl, rank]
        keep = RD.nms_ref(bb.astype(F32), lvl, thr)
        wd, ht = bb[:, 2] - bb[:, 0], bb[:, 3] - bb[:, 1]
        area = wd * ht
        for j in np.nonzero(keep)[0]:
            later = np.nonzero(lvl[j + 1:] == lvl[j])[0] + j + 1
            e = np.maximum(eb[j], eb[later])
            w = np.minimum(bb[j, 2], bb[later, 2]) - np.maximum(bb[j, 0], bb[later, 0])
            h = np.minimum(bb[j, 3], bb[later, 3]) - np.maximum(bb[j, 1], bb[later, 1])
            apart = (w < -2 * e) | (h < -2 * e)
            w, h = np.maximum(w, 0), np.maximum(h, 0)
            inter, d_inter = w * h, 2 * e * (w + h) + 4 * e * e
            d_area = 2 * e * (wd[j] + ht[j]) + 2 * e * (wd[later] + ht[later]) + 8 * e * e
            union, d_union = area[j] + area[later] - inter, d_area + d_inter
            above = (inter - d_inter) / (union + d_union) > thr
            below = (inter + d_inter) / np.maximum(union - d_union, 1e-300) < thr
            assert np.all(apart | above | below), 'seed {}: a decided pair of image {} can flip within the slack; pick another seed'.format(seed, i)
            pairs += later.shape[0]
    assert pairs > 100


def test_module_on_the_kernel_equals_the_loop(S, dev, monkeypatch):
    """`RegionProposalNetwork.forward` with the switch on against the switch off on the same precomputed head outputs: the same
    counts, boxes within 1e-3 px.  Preconditions (asserted): distinct logits, no decided IoU within 1e-3 of the threshold, no
    side within 1e-3 of min_size, adjacent distinct scores at least 1e-6 apart."""
    seed, top_n = 21, 300
    rpn, feats, images, obj, dl = rpn_and_inputs(dev, seed, top_n)
    rpn.eval()
    assert_margins(S, dev, rpn, feats, images, obj, dl, top_n, seed)
    called = []
    real = S.hip.rpn_proposals
    monkeypatch.setattr(S.hip, 'rpn_proposals', lambda *a, **k: called.append(1) or real(*a, **k))
    with torch.no_grad():
        monkeypatch.setattr(S.hip.host_policy, 'rpn_post_hip', False)
        loop, _ = rpn(images, feats)
        assert not called
        monkeypatch.setattr(S.hip.host_policy, 'rpn_post_hip', True)
        got, _ = rpn(images, feats)
        assert called == [1]
    assert len(got) == len(loop) == 2
    for g, w in zip(got, loop):
        assert g.dtype == torch.float32 and g.shape == w.shape and 10 < g.shape[0] <= top_n
        assert (g - w).abs().max().item() <= 1e-3


def test_module_in_training_mode(S, dev, monkeypatch):
    """the same with `enable_training`, K = P = 2 000: proposals as above, and the losses bit-equal (the loss path is shared: it
    reads the concatenation, which the kernel path still makes in training mode)"""
    from sc2bench_amd import detection
    seed, top_n = 24, 2000
    rpn, feats, images, obj, dl = rpn_and_inputs(dev, seed, top_n, training=True)
    detection.enable_training(rpn).train()
    assert rpn.pre_nms_top_n() == rpn.post_nms_top_n() == 2000
    assert_margins(S, dev, rpn, feats, images, obj, dl, top_n, seed)
    targets = [dict(boxes=torch.tensor([[20.0, 30.0, 90.0, 120.0], [100.0, 10.0, 180.0, 70.0]], device=dev)),
               dict(boxes=torch.tensor([[40.0, 40.0, 120.0, 100.0]], device=dev))]
    called = []
    real = S.hip.rpn_proposals
    monkeypatch.setattr(S.hip, 'rpn_proposals', lambda *a, **k: called.append(1) or real(*a, **k))
    out = {}
    for on in (False, True):
        monkeypatch.setattr(S.hip.host_policy, 'rpn_post_hip', on)
        torch.manual_seed(5)                      # (the sampler draws)
        out[on] = rpn(images, feats, targets)
    assert called == [1]
    for g, w in zip(out[True][0], out[False][0]):
        assert g.shape == w.shape and 10 < g.shape[0] <= top_n and (g - w).abs().max().item() <= 1e-3
    assert sorted(out[True][1]) == ['loss_objectness', 'loss_rpn_box_reg']
    for name in out[True][1]:
        assert out[True][1][name].requires_grad and torch.equal(out[True][1][name], out[False][1][name]), name


def test_faster_rcnn_end_to_end_on_the_kernel(S, dev, monkeypatch):
    """the full `faster_rcnn_model` once at 320 x 416: the proposals come from the kernel and the detections are well formed"""
    from sc2bench_amd import dense
    from test_detection_cpu import BACKBONE_CONFIG, MODEL_KWARGS
    torch.manual_seed(0)
    model = dense.faster_rcnn_model(BACKBONE_CONFIG, min_size=320, max_size=416, box_score_thresh=0.0, **MODEL_KWARGS)
    model.eval().to(dev)
    model.update()
    model.backbone.body.set_compute_dtype('bf16')
    model.backbone.fpn.to(torch.bfloat16)
    x = torch.rand(1, 3, 320, 416, generator=torch.Generator().manual_seed(0)).to(dev)
    seen = []
    real = S.hip.rpn_proposals

    def spy(*a, **k):
        res = real(*a, **k)
        seen.append(res.count.cpu().tolist())
        return res
    monkeypatch.setattr(S.hip, 'rpn_proposals', spy)
    monkeypatch.setattr(S.hip.host_policy, 'rpn_post_hip', True)
    with torch.no_grad():
        out = model([x[0]])
    torch.cuda.synchronize()
    assert len(seen) == 1 and 0 < seen[0][0] <= 1000
    boxes, labels, scores = out[0]['boxes'], out[0]['labels'], out[0]['scores']
    d = boxes.shape[0]
    assert 0 < d <= 100 and boxes.shape == (d, 4) and boxes.dtype == torch.float32 and labels.dtype == torch.int64
    assert torch.isfinite(boxes).all() and torch.isfinite(scores).all()
    assert labels.min() >= 1 and labels.max() <= 90 and torch.all(scores[:-1] >= scores[1:])
    assert boxes[:, 0::2].min() >= 0 and boxes[:, 0::2].max() <= 416 and boxes[:, 1::2].min() >= 0 and boxes[:, 1::2].max() <= 320
