"""sc2_seg_augment on the device against the host chain (Pillow + torch) and against tests/ref_pil_resize.py, with `torch.equal`: the
kernels are integer work up to the last two correctly rounded float32 divisions, so nothing here has a tolerance.  Outputs are written
inside NaN / sentinel arenas that are checked untouched."""
import numpy as np
import pytest
import torch

import ref_pil_resize as ref
import seg_augment_util as U

pytestmark = pytest.mark.gpu

GUARD = 4096
SENTINEL = -7777


@pytest.fixture(autouse=True)
def _switch_on(S):
    before = S.hip.host_policy.seg_augment_hip
    S.hip.configure(seg_augment_hip=True)
    yield
    S.hip.configure(seg_augment_hip=before)


def run(S, dev, samples, want_workspace=False):
    """samples -> (images, targets, status, workspace) on the host, through hip.seg_augment with both outputs inside arenas"""
    from sc2bench_amd import transforms as T
    batch = T.DeferredSegBatch(samples)
    n, (H, W) = len(samples), batch.size
    img_arena = torch.full((n * 3 * H * W + 2 * GUARD,), float('nan'), dtype=torch.float32, device=dev)
    tgt_arena = torch.full((n * H * W + 2 * GUARD,), SENTINEL, dtype=torch.int64, device=dev)
    res = S.hip.seg_augment(batch.buf.to(dev), batch.desc, batch.size, batch.mean, batch.std,
                            images_out=img_arena[GUARD:-GUARD].view(n, 3, H, W), targets_out=tgt_arena[GUARD:-GUARD].view(n, H, W),
                            return_workspace=want_workspace)
    torch.cuda.synchronize()
    img_arena, tgt_arena = img_arena.cpu(), tgt_arena.cpu()
    assert torch.isnan(img_arena[:GUARD]).all() and torch.isnan(img_arena[-GUARD:]).all()
    assert (tgt_arena[:GUARD] == SENTINEL).all() and (tgt_arena[-GUARD:] == SENTINEL).all()
    ws = res.workspace.cpu() if want_workspace else None
    return img_arena[GUARD:-GUARD].view(n, 3, H, W), tgt_arena[GUARD:-GUARD].view(n, H, W), res.status.cpu(), ws, batch


def check(S, dev, samples, host=True):
    images, targets, status, _, batch = run(S, dev, samples)
    assert status.tolist() == [0] * len(samples)
    want_images, want_targets = U.reference_batch(samples)
    for i in range(len(samples)):       # per sample, so that a failure names it
        bad = int((images[i] != want_images[i]).sum()) + int((targets[i] != want_targets[i]).sum())
        assert bad == 0, 'sample {}: {} elements differ from the restatement'.format(i, bad)
    assert torch.equal(images, want_images) and torch.equal(targets, want_targets)
    if host:
        host_images, host_targets = batch.materialize_host()
        assert torch.equal(images, host_images) and torch.equal(targets, host_targets)
    return images, targets


# ------------------------------------------------------------------------------------------------ coefficient and index tables
N_IN = list(range(1, 41)) + [333, 375, 500]


def _table_check(S, dev, T, pairs, oh, ow, axis):
    """one launch: sample k resizes `axis` n_in -> n_out (the other axis has length 1 and stays), window at the origin"""
    samples = []
    for k, (n_in, n_out) in enumerate(pairs):
        h, w, nh, nw = (1, n_in, 1, n_out) if axis == 0 else (n_in, 1, n_out, 1)
        image, mask = U.source(h, w)
        samples.append(U.sample(T, image, mask, nh, nw, flip=(axis == 0 and k % 2 == 1)))
    _, _, status, ws, _ = run(S, dev, samples, want_workspace=True)
    assert status.tolist() == [0] * len(samples)
    ws = ws.numpy()
    assert ws.shape == (len(samples), ow + oh, 12)
    for k, (n_in, n_out) in enumerate(pairs):
        if axis == 0:
            got, want = ws[k, :ow], ref.table_entries(n_in, n_out, 0, ow, n_out, flip=(k % 2 == 1))
        else:
            got, want = ws[k, ow:], ref.table_entries(n_in, n_out, 0, oh, n_out)
        assert np.array_equal(got, want), 'axis {} {} -> {}: table differs at rows {}'.format(
            axis, n_in, n_out, np.nonzero((got != want).any(1))[0][:5])


@pytest.mark.parametrize('axis', [0, 1])
def test_tables_small_outputs(S, dev, axis):
    """n_in in 1..40 and {333, 375, 500}, n_out in 1..80, wherever filterscale <= 4: where a contraction or a reciprocal would show"""
    from sc2bench_amd import transforms as T
    pairs = [(n_in, n_out) for n_in in N_IN for n_out in range(1, 81) if n_in <= 4 * n_out]
    assert len(pairs) > 3000
    # (every sample's slot is as long as the batch's longest output: 80)
    for start in range(0, len(pairs), 512):
        chunk = pairs[start:start + 512]
        longest = max(n_out for _, n_out in chunk)
        _table_check(S, dev, T, chunk, 1 if axis == 0 else longest, longest if axis == 0 else 1, axis)


@pytest.mark.parametrize('axis', [0, 1])
def test_tables_large_outputs(S, dev, axis):
    from sc2bench_amd import transforms as T
    pairs = [(n_in, n_out) for n_in in N_IN for n_out in (256, 513, 1026)]
    _table_check(S, dev, T, pairs, 1 if axis == 0 else 1026, 1026 if axis == 0 else 1, axis)


# ------------------------------------------------------------------------------------------------ window 33 x 33
def _window33_samples(T):
    samples, names = [], []

    def add(name, hw, nh, nw, top, left):
        image, mask = U.source(*hw)
        for flip in (False, True):
            samples.append(U.sample(T, image, mask, nh, nw, flip, top, left, out=33))
            names.append('{} {}x{} -> {}x{} at ({}, {}){}'.format(name, hw[0], hw[1], nh, nw, top, left, ' flipped' if flip else ''))
    # upscale (three taps): the four corners of the window's range and the middle
    for top, left in ((0, 0), (33, 69), (0, 69), (33, 0), (17, 31)):
        add('upscale', (20, 31), 66, 102, top, left)
    add('downscale near 2, padded in both', (37, 50), 18, 24, 0, 0)
    add('downscale near 4, padded in both', (37, 50), 10, 13, 0, 0)
    add('downscale near 4 on the rows only', (50, 37), 13, 37, 0, 2)
    add('horizontal pass only', (37, 50), 37, 66, 2, 30)
    add('vertical pass only', (37, 50), 60, 50, 27, 17)
    add('no pass', (50, 37), 50, 37, 17, 4)
    add('no pass', (50, 37), 50, 37, 0, 0)
    add('padded in the width', (50, 37), 40, 30, 7, 0)
    add('padded in the height', (37, 50), 30, 40, 0, 7)
    add('exact fit, no pass', (33, 33), 33, 33, 0, 0)
    add('exact height', (20, 31), 33, 51, 0, 18)
    add('exact fit, both passes', (20, 31), 33, 33, 0, 0)
    return samples, names


def test_window_33(S, dev):
    from sc2bench_amd import transforms as T
    samples, names = _window33_samples(T)
    images, targets, status, _, batch = run(S, dev, samples)
    assert status.tolist() == [0] * len(samples)
    want_images, want_targets = U.reference_batch(samples)
    host_images, host_targets = batch.materialize_host()
    assert torch.equal(want_images, host_images) and torch.equal(want_targets, host_targets)
    for i, name in enumerate(names):
        assert torch.equal(images[i], want_images[i]), name
        assert torch.equal(targets[i], want_targets[i]), name


# ------------------------------------------------------------------------------------------------ window 513 x 513
def test_window_513(S, dev):
    """the PASCAL size: short side 256 (padded right and bottom) and short side 1026 (an interior window, flipped) in one batch, so the
    16-row bands, the 64-column tiles and the per-sample descriptors run at the real tile counts"""
    from sc2bench_amd import transforms as T
    image, mask = U.source(375, 500)
    other, other_mask = U.source(375, 500, seed=1)
    samples = [U.sample(T, image, mask, 256, 341, False, 0, 0, out=513),
               U.sample(T, other, other_mask, 1026, 1368, True, 200, 500, out=513)]
    check(S, dev, samples)


# ------------------------------------------------------------------------------------------------ evaluation form
def test_evaluation_form(S, dev):
    """two samples of different resized sizes in one padded batch: the fills are 0.0f and 255; the first shrinks by 3.96 over whole
    bands (the most source rows a band can need)"""
    from sc2bench_amd import transforms as T
    a, b = U.source(281, 500), U.source(40, 75)
    samples = [U.sample(T, a[0], a[1], 71, 126), U.sample(T, b[0], b[1], 80, 150)]
    images, targets = check(S, dev, samples)
    assert images.shape == (2, 3, 80, 150)
    assert (images[0, :, 71:] == 0).all() and (images[0, :, :, 126:] == 0).all() and (targets[0, 71:] == 255).all()
    assert not torch.signbit(images[0, :, 71:]).any()


# ------------------------------------------------------------------------------------------------ mask values
def test_mask_values_survive(S, dev):
    from sc2bench_amd import transforms as T
    image, _ = U.source(37, 50)
    mask = np.resize(np.array(list(range(21)) + [255], dtype=np.uint8), (37, 50))
    full = np.full((37, 50), 255, dtype=np.uint8)
    samples = [U.sample(T, image, mask, 74, 100, False, 20, 30, out=33), U.sample(T, image, full, 74, 100, True, 20, 30, out=33),
               U.sample(T, image, mask, 37, 50, False, 0, 0, out=33)]
    images, targets = check(S, dev, samples)
    assert targets.dtype == torch.int64 and (targets[1] == 255).all()
    assert set(targets[2].flatten().tolist()) == set(range(21)) | {255}


# ------------------------------------------------------------------------------------------------ status word and fallback
def test_ratio_cap_sets_status_and_falls_back(S, dev):
    from sc2bench_amd import transforms as T
    a, b = U.source(50, 37), U.source(37, 50)
    samples = [U.sample(T, b[0], b[1], 40, 54), U.sample(T, a[0], a[1], 12, 37), U.sample(T, a[0], a[1], 13, 37)]      # 50 / 12 > 4
    _, _, status, _, batch = run(S, dev, samples)
    assert status.tolist() == [0, S.hip.SEG_AUGMENT_RATIO, 0]
    before = T.DeferredSegBatch.fallbacks
    images, targets = batch.materialize(dev)
    assert T.DeferredSegBatch.fallbacks == before + 1 and images.is_cuda
    want_images, want_targets = U.reference_batch(samples)
    assert torch.equal(images.cpu(), want_images) and torch.equal(targets.cpu(), want_targets)
    good = T.DeferredSegBatch([samples[0], samples[2]])
    images, targets = good.materialize(dev)
    assert T.DeferredSegBatch.fallbacks == before + 1
    want_images, want_targets = U.reference_batch([samples[0], samples[2]])
    assert torch.equal(images.cpu(), want_images) and torch.equal(targets.cpu(), want_targets)


# ------------------------------------------------------------------------------------------------ batch layout
def test_batch_of_one_and_of_five_sizes(S, dev):
    from sc2bench_amd import transforms as T
    sizes = ((20, 31), (37, 50), (50, 37), (33, 33), (7, 5))
    samples = []
    for k, (h, w) in enumerate(sizes):
        image, mask = U.source(h, w)
        nh, nw = T._resized_hw(h, w, 40 + 3 * k)
        samples.append(U.sample(T, image, mask, nh, nw))
    check(S, dev, samples[:1])
    check(S, dev, samples)


# ------------------------------------------------------------------------------------------------ end to end
def _loader(S, root, chain, collate, seed):
    from sc2bench_amd import config as C
    dataset = C.VOCSegmentation(str(root), image_set='train', transforms=chain)
    U.seed_all(seed)
    return torch.utils.data.DataLoader(dataset, batch_size=3, shuffle=True, num_workers=0, collate_fn=collate,
                                       generator=torch.Generator().manual_seed(seed))


def test_data_loader_and_distillation_stage(S, dev, tmp_path):
    from sc2bench_amd import training as TR, transforms as T
    import ref_seg_loss as RL
    U.write_voc_tree(tmp_path, classes=5)
    for chain, collate in ((U.train_chain(T), T.pascal_seg_eval_collate_fn), (U.eval_chain(T), T.pascal_seg_eval_collate_fn)):
        device_batches = list(_loader(S, tmp_path, chain, collate, 11))
        assert all(isinstance(b, T.DeferredSegBatch) for b in device_batches)
        S.hip.configure(seg_augment_hip=False)
        host_batches = list(_loader(S, tmp_path, chain, collate, 11))
        S.hip.configure(seg_augment_hip=True)
        assert all(isinstance(b[0], torch.Tensor) for b in host_batches) and len(host_batches) == len(device_batches) == 1
        for d, (images, targets) in zip(device_batches, host_batches):
            got = d.materialize(dev)
            assert got[0].is_cuda and torch.equal(got[0].cpu(), images) and torch.equal(got[1].cpu(), targets)
    # the train batch through the stage: the planned batch and the host's tensors give the same loss bits
    deferred = list(_loader(S, tmp_path, U.train_chain(T), T.pascal_seg_eval_collate_fn, 5))[0]
    S.hip.configure(seg_augment_hip=False)
    images, targets = list(_loader(S, tmp_path, U.train_chain(T), T.pascal_seg_eval_collate_fn, 5))[0]
    S.hip.configure(seg_augment_hip=True)
    losses = []
    for args in ((deferred,), (images.to(dev), targets.to(dev))):
        model = RL.tiny_seg_model().to(dev)
        stage = TR.DistillationStage(RL.tiny_seg_model(seed=9).to(dev), model, RL.pascal_stage_config(), dev)
        losses.append(stage.forward_process(*args).detach().cpu())
        stage.clean_modules()
    assert torch.isfinite(losses[0]) and torch.equal(losses[0], losses[1])
