"""The classification feed without a device: `Compose.plan`, `DeferredClsSample` / `DeferredClsBatch`, `cls_collate_fn`, `hip.cls_input_check`,
`config.ImageFolder` behind a data loader, and `evaluate()` on the CPU.  Everything that compares tensors compares them bit for bit."""
import os
import pickle
import random

import numpy as np
import pytest
import torch

import cls_input_util as U
import ref_cls_input as RC

Image = pytest.importorskip('PIL.Image')


@pytest.fixture(autouse=True)
def _switch_on(S):
    before = S.hip.host_policy.cls_input_hip
    S.hip.configure(cls_input_hip=True)
    yield
    S.hip.configure(cls_input_hip=before)


def pil(h, w, seed=0):
    return Image.fromarray(U.source(h, w, seed))


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_entries_are_declared_listed_and_exported(S):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'sc2_bottleneck.h')).read()
    lib = S.hip.lib()
    for name in ('sc2_cls_input', 'sc2_cls_input_workspace'):
        assert name in S.hip.ABI_SYMBOLS and name + '(' in header and hasattr(lib, name)
    assert '#define SC2_CLS_INPUT_DESC_INTS {}'.format(S.hip.CLS_INPUT_DESC_INTS) in header
    for name in ('RATIO', 'BAD', 'TAP'):
        assert '#define SC2_CLS_INPUT_{} {}'.format(name, getattr(S.hip, 'CLS_INPUT_' + name)) in header
        assert getattr(RC, name) == getattr(S.hip, 'CLS_INPUT_' + name)
    assert lib.sc2_cls_input_workspace(256, 224, 224) == 0 and lib.sc2_cls_input_workspace(0, 224, 224) == -1
    assert lib.sc2_cls_input_workspace(1, 16385, 1) == -1
    assert hasattr(S.hip.HostPolicy, 'cls_input_hip')


def test_entry_refuses_bad_arguments_before_any_launch(S):
    """SC2_REQUIRE returns before the launch, so these run without a device"""
    import ctypes
    lib = S.hip.lib()
    mean, std, zero = (ctypes.c_float * 3)(*U.MEAN), (ctypes.c_float * 3)(*U.STD), (ctypes.c_float * 3)(0.229, 0.0, 0.225)
    words = (ctypes.c_int32 * 64)()
    p = ctypes.addressof(words)
    assert lib.sc2_cls_input(p, 100, p, 0, 8, 8, mean, std, p, p, None) != 0 and '1..65535 samples' in S.hip.last_error()
    assert lib.sc2_cls_input(p, 0, p, 1, 8, 8, mean, std, p, p, None) != 0 and 'source buffer' in S.hip.last_error()
    assert lib.sc2_cls_input(p, 100, None, 1, 8, 8, mean, std, p, p, None) != 0 and 'null pointer' in S.hip.last_error()
    assert lib.sc2_cls_input(p, 100, p + 2, 1, 8, 8, mean, std, p, p, None) != 0 and 'misaligned' in S.hip.last_error()
    assert lib.sc2_cls_input(p, 100, p, 1, 8, 8, mean, zero, p, p, None) != 0 and 'std[1] is zero' in S.hip.last_error()


# ------------------------------------------------------------------------------------------------ plan: which chains
def test_plan_accepts_the_two_config_chains(S):
    from sc2bench_amd import config as C, transforms as T
    img = pil(375, 500)
    train, val = U.train_chain(C), U.eval_chain(C)
    assert isinstance(train, T.Compose) and isinstance(val, T.Compose)
    random.seed(0)
    s = train.plan(img)
    assert isinstance(s, T.DeferredClsSample) and (s.out_h, s.out_w, s.nh, s.nw) == (224, 224, 224, 224)
    assert (s.full_h, s.full_w) == s.image.shape[:2] and (s.row0, s.col0, s.top, s.left) == (0, 0, 0, 0)
    s = val.plan(img)
    assert (s.full_h, s.full_w, s.nh, s.nw, s.top, s.left, s.flip) == (375, 500, 256, 341, 16, 58, False)
    assert (s.row0, s.image.shape[0], s.col0, s.image.shape[1]) == RC.stored_box(375, 500, 256, 341, 16, 58, 224, 224)
    assert s.image.shape[0] < 375 and s.image.shape[1] < 500
    assert np.array_equal(s.image, U.source(375, 500)[s.row0:s.row0 + s.image.shape[0], s.col0:s.col0 + s.image.shape[1]])
    # Resize with an (h, w) size
    s = T.Compose([T.Resize([64, 80]), T.CenterCrop(48), T.ToTensor(), T.Normalize(U.MEAN, U.STD)]).plan(pil(100, 120))
    assert (s.full_h, s.full_w, s.nh, s.nw, s.top, s.left, s.out_h, s.out_w) == (100, 120, 64, 80, 8, 16, 48, 48)


def _near_misses(T):
    n = T.Normalize(U.MEAN, U.STD)
    rrc, flip, tt, rs, cc = T.RandomResizedCrop([24, 24]), T.RandomHorizontalFlip(0.5), T.ToTensor(), T.Resize(32), T.CenterCrop([24, 24])
    rgb, grey = pil(40, 50), Image.fromarray(U.source(40, 50)[:, :, 0])
    return [
        ('no flip', [rrc, tt, n], rgb),
        ('flip before the crop', [flip, rrc, tt, n], rgb),
        ('no normalisation', [rrc, flip, tt], rgb),
        ('something behind the normalisation', [rrc, flip, tt, n, n], rgb),
        ('bicubic crop', [T.RandomResizedCrop([24, 24], interpolation='bicubic'), flip, tt, n], rgb),
        ('nearest resize', [T.Resize(32, interpolation='nearest'), cc, tt, n], rgb),
        ('one-value mean', [rrc, flip, tt, T.Normalize([0.5], [0.5])], rgb),
        ('a zero std', [rs, cc, tt, T.Normalize(U.MEAN, (0.2, 0.0, 0.2))], rgb),
        ('a one-element Resize size', [T.Resize([32]), cc, tt, n], rgb),
        ('no centre crop', [rs, tt, n], rgb),
        ('a centre crop larger than the resized image', [rs, T.CenterCrop([24, 48]), tt, n], rgb),
        ('a grey image, train', [rrc, flip, tt, n], grey),
        ('a grey image, eval', [rs, cc, tt, n], grey),
        ('a tensor', [rrc, flip, tt, n], torch.zeros(3, 40, 50)),
        ('an array', [rs, cc, tt, n], U.source(40, 50)),
        ('a subclass of the crop', [type('Mine', (T.RandomResizedCrop,), {})([24, 24]), flip, tt, n], rgb),
    ]


def test_plan_refuses_each_near_miss_and_draws_nothing(S):
    from sc2bench_amd import transforms as T
    for name, chain, img in _near_misses(T):
        random.seed(3)
        torch.manual_seed(3)
        state, tstate = random.getstate(), torch.get_rng_state()
        assert T.Compose(chain).plan(img) is None, name
        assert random.getstate() == state and torch.equal(torch.get_rng_state(), tstate), name + ': a number was drawn'


# ------------------------------------------------------------------------------------------------ plan == __call__
def test_plan_host_equals_call_for_50_seeds(S):
    from sc2bench_amd import config as C
    train, val = U.train_chain(C, size=(24, 32)), U.eval_chain(C, resize=32, crop=(24, 28))
    sizes = ((37, 53), (53, 37), (101, 77), (20, 20), (1, 40), (40, 1), (5, 7))
    flips = 0
    for k in range(50):
        img = pil(*sizes[k % len(sizes)], seed=k)
        random.seed(k)
        want = train(img)
        after = random.getstate()
        random.seed(k)
        s = train.plan(img)
        assert random.getstate() == after, 'seed {}: plan and __call__ drew different numbers'.format(k)
        got = s.host()
        assert got.dtype == torch.float32 and got.shape == (3, 24, 32) and torch.equal(got, want), 'seed {}'.format(k)
        flips += int(s.flip)
        if min(img.size) >= 2:      # (a one-pixel side under Resize(32) makes the other side thousands of pixels long)
            e = val.plan(img)
            assert e is not None and torch.equal(e.host(), val(img)), 'seed {}: eval form'.format(k)
    assert 10 < flips < 40


def test_ten_failures_give_the_central_crop(S):
    """a 1 x 40 image: no drawn crop fits (its height would be at least 2), so the central crop at the closest ratio is taken"""
    from sc2bench_amd import config as C
    train = U.train_chain(C, size=(24, 32))
    img = pil(1, 40)
    for k in range(5):
        random.seed(k)
        s = train.plan(img)
        assert s.image.shape == (1, 1, 3) and np.array_equal(s.image[0, 0], U.source(1, 40)[0, 19])      # (h - 1) // 2, (40 - 1) // 2
        random.seed(k)
        assert torch.equal(s.host(), train(img))


def test_oversize_source_becomes_an_identity_sample(S):
    from sc2bench_amd import config as C, transforms as T
    img = pil(140, 200)
    val = U.eval_chain(C, resize=32, crop=(24, 24))       # 140 / 32 > 4
    s = val.plan(img)
    assert s.image.shape == (24, 24, 3) and (s.full_h, s.full_w, s.nh, s.nw, s.row0, s.col0, s.top, s.left, s.flip) == (24, 24, 24, 24, 0, 0, 0, 0, False)
    assert torch.equal(s.host(), val(img))
    train = T.Compose([T.RandomResizedCrop([8, 8], scale=(0.9, 1.0)), T.RandomHorizontalFlip(0.5), T.ToTensor(), T.Normalize(U.MEAN, U.STD)])
    seen = set()
    for k in range(8):
        random.seed(k)
        want = train(img)
        random.seed(k)
        s = train.plan(img)
        assert s.image.shape == (8, 8, 3) and (s.full_h, s.nh, s.flip) == (8, 8, False) and torch.equal(s.host(), want)
        random.seed(k)
        train.transforms[0].draw(140, 200)
        seen.add(train.transforms[1].draw())
    assert seen == {True, False}       # both the flipped and the unflipped finish were compared
    # exactly 4 stays with the kernel
    s = U.eval_chain(C, resize=35, crop=(24, 24)).plan(img)
    assert (s.full_h, s.nh) == (140, 35) and s.image.shape[0] > 24


# ------------------------------------------------------------------------------------------------ batch and collate
def _planned(C, n=3, seed=0):
    val = U.eval_chain(C, resize=32, crop=(24, 24))
    return [val.plan(pil(40 + 7 * k, 61 - 5 * k, seed=seed + k)) for k in range(n)], val


def test_collate_planned_plain_and_mixed(S):
    from sc2bench_amd import config as C, transforms as T
    samples, val = _planned(C)
    batch, labels = T.cls_collate_fn([(s, k) for k, s in enumerate(samples)])
    assert isinstance(batch, T.DeferredClsBatch) and len(batch) == 3 and batch.size == (24, 24)
    assert labels.dtype == torch.int64 and labels.tolist() == [0, 1, 2]
    assert batch.desc.dtype == torch.int32 and batch.desc.shape == (3, S.hip.CLS_INPUT_DESC_INTS)
    assert batch.buf.dtype == torch.uint8 and batch.buf.numel() == sum(s.image.size for s in samples)
    want = torch.stack([val(pil(40 + 7 * k, 61 - 5 * k, seed=k)) for k in range(3)])
    assert torch.equal(batch.materialize_host(), want) and torch.equal(batch.materialize(), want)
    assert torch.equal(batch.to('cpu').materialize(torch.device('cpu')), want)
    plain = [(torch.full((3, 4, 4), float(k)), k) for k in range(3)]
    images, labels = T.cls_collate_fn(plain)
    ref_images, ref_labels = torch.utils.data.default_collate(plain)
    assert torch.equal(images, ref_images) and torch.equal(labels, ref_labels)
    assert T.cls_collate_fn([{'a': 1}, {'a': 2}])['a'].tolist() == [1, 2]
    with pytest.raises(TypeError, match='mixes planned and transformed'):
        T.cls_collate_fn([(samples[0], 0), plain[1]])
    other = T.DeferredClsSample(samples[0].image, *[getattr(samples[0], k) for k in T.DeferredClsSample.__slots__[1:12]], (0.5, 0.5, 0.5), U.STD)
    with pytest.raises(ValueError, match='different normalisations'):
        T.DeferredClsBatch([samples[0], other])
    with pytest.raises(ValueError, match='different output sizes'):
        T.DeferredClsBatch([samples[0], T.DeferredClsSample.identity(U.source(8, 8), U.MEAN, U.STD)])
    assert T.COLLATE_FUNC_DICT['cls_collate_fn'] is T.cls_collate_fn


def test_batch_pickles_and_samples_round_trip(S):
    from sc2bench_amd import config as C, transforms as T
    samples, _ = _planned(C)
    samples.append(U.train_sample(T, U.source(30, 40), 2, 3, 20, 30, 24, 24, flip=True))
    batch = T.DeferredClsBatch(samples)
    for b in (batch, pickle.loads(pickle.dumps(batch))):
        back = b.samples()
        assert len(back) == len(b) == 4
        for s, t in zip(samples, back):
            assert np.array_equal(s.image, t.image)
            assert all(getattr(s, k) == getattr(t, k) for k in T.DeferredClsSample.__slots__[1:])
        assert torch.equal(b.materialize_host(), batch.materialize_host())
    one = pickle.loads(pickle.dumps(samples[3]))
    assert one.flip is True and np.array_equal(one.image, samples[3].image) and torch.equal(one.host(), samples[3].host())
    assert batch.pin_memory is not None and callable(batch.to)


# ------------------------------------------------------------------------------------------------ the host check
def test_check_names_each_bad_field(S):
    hip = S.hip
    good = dict(offset=0, h=10, w=12, full_h=20, full_w=24, row0=5, col0=6, nh=16, nw=18, flip=0, top=2, left=3)
    nbytes = 3 * 10 * 12
    table = np.stack([hip.cls_input_desc(**good)])
    assert hip.cls_input_check(table, nbytes, 8, 8) is not None
    assert hip.cls_input_desc(offset=7, h=3, w=4, nh=8, nw=8).tolist()[:12] == [7, 3, 4, 3, 4, 0, 0, 8, 8, 0, 0, 0]
    cases = [
        (dict(h=0), 'h = 0: sides are 1..16384'), (dict(w=16385), 'w = 16385: sides'), (dict(full_h=0), 'full_h = 0: sides'),
        (dict(full_w=-1), 'full_w = -1: sides'), (dict(nh=0), 'nh = 0: sides'), (dict(nw=20000), 'nw = 20000: sides'),
        (dict(offset=-1), 'offset = -1: the stored box lies outside the buffer of 360 bytes'),
        (dict(offset=1), 'offset = 1: the stored box lies outside the buffer'),
        (dict(row0=11), 'row0 = 11: the stored box of 10 lies outside the full image of 20'),
        (dict(row0=-1), 'row0 = -1: the stored box'), (dict(col0=13), 'col0 = 13: the stored box of 12 lies outside the full image of 24'),
        (dict(flip=2), 'flip = 2: 0 or 1'), (dict(top=9), 'top = 9: the window of 8 lies outside the resized image of 16'),
        (dict(top=-1), 'top = -1: the window'), (dict(left=11), 'left = 11: the window of 8 lies outside the resized image of 18'),
    ]
    for change, message in cases:
        rows = np.stack([hip.cls_input_desc(**good), hip.cls_input_desc(**dict(good, **change))])
        with pytest.raises(ValueError) as e:
            hip.cls_input_check(rows, nbytes, 8, 8)
        assert 'cls_input: sample 1: ' + message in str(e.value), (change, str(e.value))
    for bad_table in (np.zeros((0, 16), np.int32), np.zeros((2, 12), np.int32), np.zeros(16, np.int32)):
        with pytest.raises(ValueError, match='a descriptor table'):
            hip.cls_input_check(bad_table, nbytes, 8, 8)
    with pytest.raises(ValueError, match='output slot'):
        hip.cls_input_check(table, nbytes, 0, 8)
    with pytest.raises(ValueError, match='a source buffer of 0 bytes'):
        hip.cls_input_check(table, 0, 8, 8)
    # a ratio above 4 and a box that misses a tap are well formed: the kernel's status word answers them
    hip.cls_input_check(np.stack([hip.cls_input_desc(**dict(good, full_h=100, row0=0))]), nbytes, 8, 8)
    hip.cls_input_check(np.stack([hip.cls_input_desc(**dict(good, h=1, w=1))]), nbytes, 8, 8)


# ------------------------------------------------------------------------------------------------ dataset, loader, evaluate
def _loader(S, root, chain, workers, seed=7, via_config=False):
    from sc2bench_amd import config as C, evaluation as E, transforms as T
    dataset = C.ImageFolder(str(root), transform=chain, plan_samples=not via_config)
    if via_config:
        return E.build_data_loader({'d': dataset}, {'dataset_id': 'd', 'kwargs': {'batch_size': 4, 'num_workers': workers}})
    U.seed_all(seed)
    return torch.utils.data.DataLoader(dataset, batch_size=4, num_workers=workers, collate_fn=T.cls_collate_fn)


def E_build(S, root, chain, collate):
    from sc2bench_amd import config as C, evaluation as E
    return E.build_data_loader({'d': C.ImageFolder(str(root), transform=chain)}, {'dataset_id': 'd', 'collate_fn': collate, 'kwargs': {'batch_size': 4}})


def test_image_folder_behind_a_data_loader_with_workers(S, tmp_path):
    from sc2bench_amd import config as C, transforms as T
    files = U.write_image_tree(tmp_path)
    val = U.eval_chain(C, resize=32, crop=(24, 24))
    want = [(val(Image.open(path).convert('RGB')), label) for path, label in files]
    planned = list(_loader(S, tmp_path, val, 2))
    assert [type(b[0]) for b in planned] == [T.DeferredClsBatch] * 2 and [len(b[0]) for b in planned] == [4, 2]
    got = torch.cat([b[0].materialize() for b in planned])
    assert torch.equal(got, torch.stack([w[0] for w in want])) and torch.cat([b[1] for b in planned]).tolist() == [w[1] for w in want]
    S.hip.configure(cls_input_hip=False)
    plain = list(_loader(S, tmp_path, val, 2))
    S.hip.configure(cls_input_hip=True)
    assert all(isinstance(b[0], torch.Tensor) for b in plain) and torch.equal(torch.cat([b[0] for b in plain]), got)
    # a loader that names no collate function gets this one from build_data_loader
    built = _loader(S, tmp_path, val, 0, via_config=True)
    assert built.collate_fn is T.cls_collate_fn and built.dataset.plan_samples and isinstance(next(iter(built))[0], T.DeferredClsBatch)
    # ... and a loader that names one, like `dataset[i]` by hand, keeps getting tensors
    named = E_build(S, tmp_path, val, 'default_collate_w_pil')
    assert not named.dataset.plan_samples and isinstance(next(iter(named))[0], torch.Tensor)
    assert isinstance(C.ImageFolder(str(tmp_path), transform=val)[0][0], torch.Tensor)
    assert isinstance(C.ImageFolder(str(tmp_path), transform=val, plan_samples=True)[0][0], T.DeferredClsSample)
    # the train chain in the main process: the same draws either way
    train = U.train_chain(C, size=(24, 24))
    planned = list(_loader(S, tmp_path, train, 0, seed=11))
    S.hip.configure(cls_input_hip=False)
    plain = list(_loader(S, tmp_path, train, 0, seed=11))
    S.hip.configure(cls_input_hip=True)
    assert isinstance(planned[0][0], T.DeferredClsBatch)
    assert torch.equal(torch.cat([b[0].materialize() for b in planned]), torch.cat([b[0] for b in plain]))


def test_evaluate_on_the_cpu_is_the_same_either_way(S, tmp_path):
    from sc2bench_amd import config as C, evaluation as E
    U.write_image_tree(tmp_path, classes=3, per_class=3)
    val = U.eval_chain(C, resize=32, crop=(24, 24))
    model = U.TinyClassifier()
    results = []
    for on in (True, False):
        S.hip.configure(cls_input_hip=on)
        results.append(E.evaluate(model, _loader(S, tmp_path, val, 0), torch.device('cpu'), log_freq=0))
    S.hip.configure(cls_input_hip=True)
    assert results[0]['samples'] == results[1]['samples'] == 9
    assert results[0]['acc1'] == results[1]['acc1'] and results[0]['acc5'] == results[1]['acc5']
    limited = E.evaluate(model, _loader(S, tmp_path, val, 0), torch.device('cpu'), max_samples=4, log_freq=0)
    assert limited['samples'] == 4


def test_to_device_passes_a_planned_batch_through(S):
    from sc2bench_amd import config as C, training as TR, transforms as T
    samples, _ = _planned(C)
    batch = T.DeferredClsBatch(samples)
    moved = TR._to_device((batch, torch.zeros(3)), torch.device('cpu'))
    assert moved[0] is batch and batch.device == torch.device('cpu')
