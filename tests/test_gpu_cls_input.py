"""sc2_cls_input on the device against tests/ref_cls_input.py and against the host chain (Pillow + torch), with `torch.equal`: the kernel
is integer work up to the last two correctly rounded float32 divisions, so nothing here has a tolerance.  Outputs are written inside a
NaN arena whose borders are checked untouched.  Shapes: the smallest at which 16 x 64 tiles and nine taps can go wrong."""
import pytest
import torch

import cls_input_util as U
import ref_cls_input as RC

pytestmark = pytest.mark.gpu

GUARD = 4096
OUT = (40, 72)      # more than one tile each way, a multiple of neither 16 nor 64


@pytest.fixture(autouse=True)
def _switch_on(S):
    before = S.hip.host_policy.cls_input_hip
    S.hip.configure(cls_input_hip=True)
    yield
    S.hip.configure(cls_input_hip=before)


def launch(S, dev, batch, desc=None):
    """-> (images [n,3,H,W] on the host with NaN where nothing was written, status list): hip.cls_input into a NaN arena"""
    n, (H, W) = len(batch), batch.size
    arena = torch.full((n * 3 * H * W + 2 * GUARD,), float('nan'), dtype=torch.float32, device=dev)
    res = S.hip.cls_input(batch.buf.to(dev), batch.desc if desc is None else desc, batch.size, batch.mean, batch.std,
                          images_out=arena[GUARD:-GUARD].view(n, 3, H, W))
    torch.cuda.synchronize()
    arena = arena.cpu()
    assert torch.isnan(arena[:GUARD]).all() and torch.isnan(arena[-GUARD:]).all(), 'a write outside the output'
    return arena[GUARD:-GUARD].view(n, 3, H, W), res.status.cpu().tolist()


def check(S, dev, samples, names=None, host=True):
    from sc2bench_amd import transforms as T
    batch = T.DeferredClsBatch(samples)
    images, status = launch(S, dev, batch)
    assert status == [0] * len(samples)
    want = U.reference_batch(samples)
    for i in range(len(samples)):       # per sample, so that a failure names it
        bad = int((images[i] != want[i]).sum())
        assert bad == 0, 'sample {} ({}): {} elements differ from the restatement'.format(i, names[i] if names else '', bad)
    assert torch.equal(images, want)
    if host:
        assert torch.equal(batch.materialize_host(), want)
    return images


# ------------------------------------------------------------------------------------------------ a window larger than a tile
@pytest.mark.parametrize('hw', [(37, 53), (160, 288), (157, 281)], ids=['37x53', '160x288-ratio-4', '157x281-ratio-3.9'])
@pytest.mark.parametrize('flip', [False, True], ids=['plain', 'flipped'])
def test_window_larger_than_a_tile(S, dev, hw, flip):
    from sc2bench_amd import transforms as T
    image = U.source(*hw)
    check(S, dev, [U.train_sample(T, image, 0, 0, hw[0], hw[1], OUT[0], OUT[1], flip)])


def test_upscaling(S, dev):
    from sc2bench_amd import transforms as T
    image = U.source(20, 31)
    check(S, dev, [U.train_sample(T, image, 3, 4, 5, 7, OUT[0], OUT[1], flip) for flip in (False, True)])


def test_evaluation_form_with_a_trimmed_box(S, dev):
    """101 x 77 -> Resize(48) -> CenterCrop(40): the box starts inside the image on both axes"""
    from sc2bench_amd import transforms as T
    image = U.source(101, 77)
    trimmed, whole = U.eval_sample(T, image, 48, 40, 40), U.eval_sample(T, image, 48, 40, 40, trimmed=False)
    assert trimmed.row0 > 0 and trimmed.col0 > 0 and trimmed.image.shape[0] < 101 and trimmed.image.shape[1] < 77
    assert (trimmed.nh, trimmed.nw, trimmed.top, trimmed.left) == (62, 48, 11, 4)
    images = check(S, dev, [trimmed, whole])
    assert torch.equal(images[0], images[1])
    # both axes as they are (60 x 48 under Resize(48)): the identity pass reads no neighbour, so the box is exactly the window
    same = U.eval_sample(T, U.source(60, 48), 48, 40, 32)
    assert same.image.shape == (40, 32, 3) and (same.row0, same.col0, same.nh, same.nw) == (10, 8, 60, 48)
    images = check(S, dev, [same])
    assert torch.equal(images[0], torch.from_numpy(RC.normalize(U.source(60, 48)[10:50, 8:40], U.MEAN, U.STD)))


# ------------------------------------------------------------------------------------------------ a mixed batch
def _mixed(T):
    a, b, c = U.source(37, 53), U.source(160, 288), U.source(157, 281)
    samples = [
        ('37x53', U.train_sample(T, a, 0, 0, 37, 53, OUT[0], OUT[1])),
        ('160x288 flipped, ratio 4', U.train_sample(T, b, 0, 0, 160, 288, OUT[0], OUT[1], True)),
        ('157x281, ratio 3.9', U.train_sample(T, c, 0, 0, 157, 281, OUT[0], OUT[1])),
        ('5x7 upscaled, flipped', U.train_sample(T, U.source(20, 31), 3, 4, 5, 7, OUT[0], OUT[1], True)),
        ('evaluation form, trimmed', U.eval_sample(T, U.source(101, 150), 50, OUT[0], OUT[1])),
        ('identity', T.DeferredClsSample.identity(U.source(*OUT), U.MEAN, U.STD)),
        ('rows as they are, columns 2.5', U.train_sample(T, U.source(44, 190), 2, 5, 40, 180, OUT[0], OUT[1])),
    ]
    return [s for _, s in samples], [n for n, _ in samples]


def test_mixed_batch_equals_each_sample_alone(S, dev):
    from sc2bench_amd import transforms as T
    samples, names = _mixed(T)
    assert samples[4].row0 > 0 or samples[4].col0 > 0
    together = check(S, dev, samples, names)
    for i, s in enumerate(samples):
        alone, status = launch(S, dev, T.DeferredClsBatch([s]))
        assert status == [0] and torch.equal(alone[0], together[i]), names[i]
    assert torch.equal(together[5], torch.from_numpy(RC.normalize(U.source(*OUT), U.MEAN, U.STD)))


def test_stored_box_at_the_end_of_the_buffer(S, dev):
    """the last pixel of the buffer is read byte by byte (a four-byte load there would leave the buffer): a 3 x 3 box is the whole
    27-byte buffer, and the last box of a longer buffer ends it"""
    from sc2bench_amd import transforms as T
    small = U.train_sample(T, U.source(3, 3), 0, 0, 3, 3, 8, 8)
    batch = T.DeferredClsBatch([small])
    assert batch.buf.numel() == 27
    images, status = launch(S, dev, batch)
    assert status == [0] and torch.equal(images, U.reference_batch([small]))
    samples = [U.train_sample(T, U.source(9, 11), 0, 0, 9, 11, 8, 8), U.train_sample(T, U.source(7, 5), 0, 0, 7, 5, 8, 8, True)]
    batch = T.DeferredClsBatch(samples)
    assert int(batch.desc[1, 0]) + 3 * 7 * 5 == batch.buf.numel()
    check(S, dev, samples)


# ------------------------------------------------------------------------------------------------ the ImageNet size
def test_full_size_in_both_forms(S, dev):
    from sc2bench_amd import transforms as T
    sources = [U.source(375, 500, seed=k) for k in range(3)]
    train = [U.train_sample(T, sources[0], 40, 61, 288, 301, 224, 224), U.train_sample(T, sources[1], 0, 0, 375, 500, 224, 224, True),
             U.train_sample(T, sources[2], 100, 200, 90, 120, 224, 224)]
    check(S, dev, train)
    evals = [U.eval_sample(T, image, 256, 224, 224) for image in sources]
    assert all(s.image.shape[0] < 375 and s.image.shape[1] < 500 for s in evals)
    check(S, dev, evals)


# ------------------------------------------------------------------------------------------------ status words
def test_status_words_leave_the_slot_unwritten_and_fall_back(S, dev):
    """well-formed descriptors that the kernel's own checks refuse: nothing faults, nothing is written, the batch goes to the host"""
    from sc2bench_amd import transforms as T
    hip = S.hip
    good = U.train_sample(T, U.source(37, 53), 0, 0, 37, 53, OUT[0], OUT[1])
    over = U.train_sample(T, U.source(161, 60), 0, 0, 161, 60, OUT[0], OUT[1])            # 161 > 4 * 40: past the ratio cap
    trimmed = U.eval_sample(T, U.source(101, 150), 50, OUT[0], OUT[1])
    last = U.train_sample(T, U.source(44, 190), 2, 5, 40, 180, OUT[0], OUT[1], True)
    samples = [good, over, trimmed, last]
    batch = T.DeferredClsBatch(samples)
    desc = batch.desc.clone()
    f = {name: k for k, name in enumerate(hip.CLS_INPUT_FIELDS)}
    desc[2, f['h']] -= 1                                                                  # the box loses its last row: a tap outside it
    images, status = launch(S, dev, batch, desc)
    assert status == [0, hip.CLS_INPUT_RATIO, hip.CLS_INPUT_TAP, 0]
    assert torch.isnan(images[1]).all() and torch.isnan(images[2]).all()
    assert torch.equal(images[0], U.reference(good)) and torch.equal(images[3], U.reference(last))
    # a box that starts one column late, and one that ends one column early
    for field, delta in (('col0', 1), ('w', -1), ('row0', 1)):
        desc = batch.desc.clone()
        desc[2, f[field]] += delta
        if field in ('col0', 'row0'):     # (keep the box inside the full image: it shrinks by what it moves)
            desc[2, f['w' if field == 'col0' else 'h']] -= 1
        images, status = launch(S, dev, batch, desc)
        assert status == [0, hip.CLS_INPUT_RATIO, hip.CLS_INPUT_TAP, 0], field
        assert torch.isnan(images[2]).all() and torch.equal(images[3], U.reference(last)), field
    # materialize: one flagged sample sends the batch to the host path, which Pillow finishes whatever the ratio
    before = T.DeferredClsBatch.fallbacks
    got = batch.materialize(dev)
    assert T.DeferredClsBatch.fallbacks == before + 1 and got.is_cuda
    assert torch.equal(got.cpu(), batch.materialize_host())
    assert torch.equal(got[0].cpu(), U.reference(good)) and torch.equal(got[2].cpu(), U.reference(trimmed))
    clean = T.DeferredClsBatch([good, trimmed, last])
    got = clean.materialize(dev)
    assert T.DeferredClsBatch.fallbacks == before + 1 and torch.equal(got.cpu(), U.reference_batch([good, trimmed, last]))


# ------------------------------------------------------------------------------------------------ end to end
def _loader(S, root, chain, seed):
    from sc2bench_amd import config as C, evaluation as E
    U.seed_all(seed)
    return E.build_data_loader({'d': C.ImageFolder(str(root), transform=chain)}, {'dataset_id': 'd', 'kwargs': {'batch_size': 4, 'num_workers': 0}})


def test_data_loader_evaluate_and_distillation_stage(S, dev, tmp_path):
    from sc2bench_amd import config as C, evaluation as E, training as TR, transforms as T
    U.write_image_tree(tmp_path, classes=3, per_class=3)
    val, train = U.eval_chain(C, resize=32, crop=(24, 32)), U.train_chain(C, size=(24, 40))
    model = U.TinyClassifier().to(dev)
    logits = {True: [], False: []}
    results = {}
    for on in (True, False):
        S.hip.configure(cls_input_hip=on)
        hook = model.register_forward_hook(lambda m, i, o, on=on: logits[on].append(o.detach().cpu()))
        first = next(iter(_loader(S, tmp_path, val, 3)))[0]
        assert isinstance(first, T.DeferredClsBatch if on else torch.Tensor)
        results[on] = E.evaluate(model, _loader(S, tmp_path, val, 3), dev, log_freq=0)
        hook.remove()
    S.hip.configure(cls_input_hip=True)
    assert results[True]['samples'] == results[False]['samples'] == 9 and len(logits[True]) == len(logits[False]) == 3
    assert all(torch.equal(a, b) for a, b in zip(logits[True], logits[False]))
    assert results[True]['acc1'] == results[False]['acc1'] and results[True]['acc5'] == results[False]['acc5']
    # one training step's forward: the planned batch and the host's tensors give the same loss bits
    before = T.DeferredClsBatch.fallbacks
    deferred, labels = next(iter(_loader(S, tmp_path, train, 5)))
    S.hip.configure(cls_input_hip=False)
    images, _ = next(iter(_loader(S, tmp_path, train, 5)))
    S.hip.configure(cls_input_hip=True)
    assert isinstance(deferred, T.DeferredClsBatch) and isinstance(images, torch.Tensor)
    assert torch.equal(deferred.materialize(dev).cpu(), images)
    losses = []
    for batch in (TR._to_device(deferred, dev), images.to(dev)):
        student = U.TinyClassifier(seed=9).to(dev)
        for p in student.parameters():
            p.requires_grad_(True)
        stage = TR.DistillationStage(U.TinyClassifier().to(dev), student, U.stage_config(), dev)
        losses.append(stage.forward_process(batch, labels.to(dev)).detach().cpu())
        stage.clean_modules()
    assert torch.isfinite(losses[0]) and losses[0] > 0 and torch.equal(losses[0], losses[1])
    assert T.DeferredClsBatch.fallbacks == before
