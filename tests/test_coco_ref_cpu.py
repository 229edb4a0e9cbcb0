"""tests/ref_coco.py, the sequential restatement of COCOeval's bbox protocol, proven on cases whose statistics are derived on
paper.  No pycocotools output exists to compare with (it is not installable here): fidelity rests on these cases.

Notation: P1 = 1 / (1 + 2^-52) = 0.9999999999999998, the precision of a single true positive (pr = tp / (fp + tp + spacing(1)); for
tp + fp >= 2 the spacing is rounded away).  stats = (AP, AP50, AP75, APs, APm, APl, AR1, AR10, AR100, ARs, ARm, ARl).  A mean over
equal values v is compared with a relative 1e-12 (numpy's pairwise sum of n copies of v is not bit-for-bit n * v)."""
import numpy as np
import pytest

from tests import coco_cases as C
from tests import ref_coco as R

P1 = 1.0 / (1.0 + 2.0 ** -52)


def close(got, want):
    return got == pytest.approx(want, rel=1e-12, abs=0)


def test_tables():
    assert R.IOU_THRS[0] == 0.5 and R.IOU_THRS[5] == 0.75 and len(R.IOU_THRS) == 10 and R.IOU_THRS[-1] == pytest.approx(0.95)
    assert R.REC_THRS[0] == 0.0 and R.REC_THRS[50] == 0.5 and R.REC_THRS[100] == 1.0 and len(R.REC_THRS) == 101


def test_perfect_detections():
    """Four ground truths (areas 100, 2500, 40000, 400) each with an identical detection: every detection is a true positive at every
    threshold, in every area range that holds a ground truth (in the other ranges the pair is ignored together).  pr is P1 after the
    first true positive of a curve and exactly 1 from the second on; the running maximum from the right keeps P1 only where a
    curve has a single entry.  Every populated precision is P1 or 1, every recall 1 -- except AR1: one detection per image finds 2 of
    4 ground truths (0.5)."""
    r = R.evaluate(*C.perfect())
    p = r['precision']
    assert (p > -1).all()      # small, medium and large all hold a ground truth
    assert set(np.unique(p[..., 1:]).tolist()) <= {P1, 1.0}      # maxDets 10 and 100 (one detection per image reaches half the recalls)
    assert (r['recall'][:, :, :, 1:] == 1.0).all()
    assert (r['recall'][:, 0, 0, 0] == 0.5).all()
    assert all(abs(v - 1.0) <= 2.0 ** -52 for v in r['stats'][[0, 1, 2, 3, 4, 5]])
    assert r['stats'][6] == 0.5 and (r['stats'][7:] == 1.0).all()


def test_tp_fp_tp_interpolation():
    """Two large ground truths; detections in score order: TP (IoU 1), FP (no overlap), TP (IoU 1), the same at all ten thresholds.
      tp = 1 1 2, fp = 0 1 1, rc = .5 .5 1, pr = P1, 1/2, 2/3 -> non-increasing from the right: P1, 2/3, 2/3.
      recThrs 0 .. 0.50 (51 values) first reach rc at entry 0 -> P1; 0.51 .. 1 (50 values) at entry 2 -> 2/3.
      AP = AP50 = AP75 = APl = (51 P1 + 50 * 2/3) / 101 = 0.834983...;  small / medium hold no ground truth: -1.
      AR1 = 1/2 (the first detection alone), AR10 = AR100 = ARl = 1."""
    r = R.evaluate(*C.tp_fp_tp())
    row = r['precision'][0, :, 0, 0, 2]
    assert (row[:51] == P1).all() and (row[51:] == 2.0 / 3.0).all()
    ap = (51 * P1 + 50 * (2.0 / 3.0)) / 101
    s = r['stats']
    assert close(s[0], ap) and close(s[1], ap) and close(s[2], ap) and close(s[5], ap)
    assert s[3] == -1 and s[4] == -1 and s[9] == -1 and s[10] == -1
    assert s[6] == 0.5 and s[7] == 1.0 and s[8] == 1.0 and s[11] == 1.0
    assert r['lines'][0] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.835'
    assert r['lines'][8] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 1.000'
    assert r['lines'][1] == ' Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = 0.835'


def test_crowd_matched_twice_counts_neither():
    """A crowd ground truth holding two detections (IoU against a crowd = intersection / detection area = 1) and one plain ground truth
    with its detection, scored below them.  Both crowd matches are ignored: tp = 0 0 1, fp = 0 0 0 -> pr ends at P1, AP = P1 (as false
    positives they would give 1/3).  AR1 = 0: the single kept detection is an ignored one."""
    r = R.evaluate(*C.crowd_twice())
    matched, ignored, npig, which = r['matches'][(1, 1)]
    assert [which[0][0][d] for d in range(3)] == [0, 0, 1] and [ignored[0][0][d] for d in range(3)] == [1, 1, 0]
    assert npig[0] == 1
    assert (r['precision'][:, :, 0, 0, 2] == P1).all() and r['stats'][6] == 0.0 and r['stats'][8] == 1.0


def test_out_of_range_ground_truth_absorbs_detection():
    """Annotation 1: a 30 x 30 box whose `area` field says 2000 (medium; the field decides, not the box), annotation 2: 10 x 10 (small).
    In the small range annotation 1 is ignored and absorbs its detection (score .9): tp = 0 1, fp = 0 0 -> APs = P1; as a false positive
    it would give 1/2.  In the medium range the roles swap: APm = P1.  No large ground truth: APl = -1."""
    r = R.evaluate(*C.absorbed_by_out_of_range_gt())
    s = r['stats']
    assert close(s[3], P1) and close(s[4], P1) and s[5] == -1
    assert r['matches'][(1, 1)][2] == [2, 1, 1, 0]


def test_unmatched_small_detection_ignored_in_large_range():
    """A 10 x 10 detection (score .9) that matches nothing, then the large ground truth's detection (score .5).
    All areas: tp = 0 1, fp = 1 1, pr = 0, 1/2 -> 1/2, 1/2; rc = 0, 1: AP = 1/2.  Large range: the small detection's own area (100) is
    below 96^2, so it is ignored: APl = P1."""
    r = R.evaluate(*C.small_unmatched_in_large())
    assert (r['precision'][:, :, 0, 0, 2] == 0.5).all() and r['stats'][0] == 0.5
    assert (r['precision'][:, :, 0, 3, 2] == P1).all()


def test_equal_iou_moves_match_to_later_ground_truth():
    """Two identical ground truths and two identical detections: IoU 1 against both; `iou < best` does not skip an equal IoU, so the first
    detection ends on ground truth 1 and the second takes ground truth 0."""
    r = R.evaluate(*C.equal_iou_later_gt())
    which = r['matches'][(1, 1)][3]
    assert all(which[0][t] == [1, 0] for t in range(10))
    assert r['stats'][8] == 1.0


def test_non_ignored_match_is_kept():
    """One detection: IoU 60/100 with the plain ground truth (listed first) and 1 with the crowd.  At thresholds .5, .55, .6 the plain
    ground truth matches and the walk stops at the ignored crowd; from .65 on only the crowd matches (ignored).  AP = 3/10 * P1."""
    r = R.evaluate(*C.keep_non_ignored_match())
    matched, ignored, npig, which = r['matches'][(1, 1)]
    assert [which[0][t][0] for t in range(10)] == [0, 0, 0] + [1] * 7
    assert [ignored[0][t][0] for t in range(10)] == [0, 0, 0] + [1] * 7
    assert close(r['stats'][0], 0.3 * P1) and close(r['stats'][1], P1) and r['stats'][2] == 0.0


def test_101_detections_cut_to_100():
    """100 false positives scored above the one detection that fits the ground truth: the 101st of the image's category is dropped before
    matching.  tp stays 0: AP = 0, AR100 = 0."""
    r = R.evaluate(*C.cut_to_100())
    assert len(r['segments'][(1, 1)][0]) == 100
    assert r['stats'][0] == 0.0 and r['stats'][8] == 0.0


def test_max_det_cuts():
    """Eleven ground truths, each with an identical detection: the first 1 / 10 / 100 detections find 1 / 10 / 11 of them:
    AR1 = 1/11, AR10 = 10/11, AR100 = 1."""
    r = R.evaluate(*C.max_det_cuts())
    assert (r['recall'][:, 0, 0] == np.array([1.0 / 11.0, 10.0 / 11.0, 1.0])).all()
    assert close(r['stats'][6], 1.0 / 11.0) and close(r['stats'][7], 10.0 / 11.0) and r['stats'][8] == 1.0


def test_image_without_predictions_lowers_recall():
    """Two images with one ground truth each; image 2 is evaluated with an empty prediction.  npig = 2, tp = 1: rc = 1/2, pr = P1.
    recThrs 0 .. 0.5 (51 values) -> P1, the other 50 -> 0: AP = 51 P1 / 101; AR = 1/2."""
    r = R.evaluate(*C.image_without_predictions())
    assert r['img_ids'] == [1, 2]
    assert close(r['stats'][0], 51 * P1 / 101) and r['stats'][8] == 0.5


def test_category_without_ground_truth_is_left_out():
    """Category 2 has a detection and no ground truth: -1 everywhere, left out of the means, which are category 1's (P1 and 1)."""
    r = R.evaluate(*C.category_without_gt())
    assert (r['precision'][:, :, 1] == -1).all() and (r['recall'][:, 1] == -1).all()
    assert close(r['stats'][0], P1) and r['stats'][8] == 1.0


def test_label_outside_categories_is_dropped():
    """Detections labelled 99, 2 and 0 (the categories are 1 and 3) score above the true positive and vanish: AP = P1."""
    r = R.evaluate(*C.label_outside_categories())
    assert len(r['segments'][(1, 1)][0]) == 1 and len(r['segments'][(1, 3)][0]) == 0
    assert close(r['stats'][0], P1) and (r['precision'][:, :, 1] == -1).all()


def test_iou_exactly_on_threshold_matches():
    """A detection covering exactly half of the ground truth and nothing else: IoU = 5000 / 10000 = 0.5 = iouThrs[0]: a match at .5 (best
    starts AT the threshold and only a smaller IoU is skipped), none from .55 on: AP50 = P1, AP75 = 0, AP = P1 / 10."""
    r = R.evaluate(*C.iou_on_threshold())
    assert R.iou([0.0, 0.0, 100.0, 50.0], [0.0, 0.0, 100.0, 100.0], False) == 0.5
    matched = r['matches'][(1, 1)][0]
    assert [matched[0][t][0] for t in range(10)] == [1] + [0] * 9
    assert close(r['stats'][1], P1) and r['stats'][2] == 0.0 and close(r['stats'][0], P1 / 10)


def test_flag_words():
    r = R.evaluate(*C.keep_non_ignored_match())
    matched, ignored = r['matches'][(1, 1)][:2]
    # all areas and small (the detection's area, 100): matched at all ten, ignored at the last seven; medium / large: also ignored where
    # the plain ground truth (area 60: out of range there, hence ignored) is the match
    assert R.flag_words(matched, ignored, 0) == [1023 | (0b1111111000 << 10)] * 2 + [1023 | (1023 << 10)] * 2
