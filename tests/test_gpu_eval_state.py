"""-m gpu: the evaluation forward after the model has lived a while.  The captured bs-1 graphs (graphs.py) and the caches of folded /
packed weights keyed on the model's tensors must give what a COLD model gives: a fresh instance (built from another seed, so a key
the load misses shows up), loaded with the same state, run eagerly (`eval_graphs=False`) without any forward before.  The cases are
the ones a real evaluation meets: allocations between capture and replay, a graph captured under evaluate()'s inference mode and
replayed under no_grad, parameters replaced instead of written, several captured input shapes alive at once."""
import copy
import gc
import weakref

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def bench_mod():
    import bench
    return bench


def cold_outputs(model, build, xs, body=False):
    """`model`'s state in a fresh instance `build(seed)` that has never run a forward, run eagerly on each input of `xs` (`body`:
    and its feature-extraction body).  Its parameters are perturbed before the load (the workload builders seed themselves):
    a key the load misses shows."""
    from sc2bench_amd import hip
    sd = copy.deepcopy(model.state_dict())      # (SplittableResNet.load_state_dict pops the bottleneck keys from the dict it gets)
    cold = build(1234)
    g = torch.Generator().manual_seed(1234)
    with torch.no_grad():
        for p in cold.parameters():
            p.add_(torch.randn(p.shape, generator=g).to(p.device, p.dtype))
    cold.load_state_dict(sd)
    was = hip.host_policy.eval_graphs
    hip.configure(eval_graphs=False)
    try:
        with torch.no_grad():
            out = [cold(x) for x in xs]
            return (out, [cold._body()(x) for x in xs]) if body else out
    finally:
        hip.configure(eval_graphs=was)


def _assert_equal(got, ref, what):
    if isinstance(ref, dict):
        assert list(got) == list(ref), what
        for k in ref:
            _assert_equal(got[k], ref[k], '{}[{}]'.format(what, k))
        return
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    assert torch.equal(got, ref), '{}: warm output != cold model (max diff {})'.format(what, (got.float() - ref.float()).abs().max().item())


def _assert_close(got, ref, what):
    """the dense models' and input-compression classifiers' torch ops (MIOpen) may pick another solver between a first and a later
    call of a shape: equal to a bf16 / f32 rounding step (the tolerance of test_gpu_pipeline.py's whole-model comparison)"""
    if isinstance(ref, dict):
        assert list(got) == list(ref), what
        for k in ref:
            _assert_close(got[k], ref[k], '{}[{}]'.format(what, k))
        return
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    scale = ref.float().abs().max().item()
    diff = (got.float() - ref.float()).abs().max().item()
    assert diff <= 2.0 ** -6 * scale + 1e-6, '{}: warm output != cold model (max diff {}, scale {})'.format(what, diff, scale)


def _like(w, v):
    """`v` as a fresh tensor with `w`'s dtype, device and memory format"""
    return torch.empty_like(w).copy_(v)


# ---- 1. every address a captured graph holds is owned by the graph or the model

def test_every_address_a_graph_holds_is_owned(S, dev, bench_mod, monkeypatch):
    from sc2bench_amd import hip
    from sc2bench_amd.graphs import EvalGraphs
    model = bench_mod.build_model(dev)
    x = bench_mod.synthetic_batch(1, dev, seed=3)
    with torch.no_grad():
        model(x)       # (the eager forward builds the packed weights first: a capture cannot allocate them)
    seen = []
    ptr = hip._ptr

    def recording_ptr(t):
        if t is not None and torch.cuda.is_current_stream_capturing():
            seen.append((weakref.ref(t), t.data_ptr(), tuple(t.shape)))
        return ptr(t)

    monkeypatch.setattr(hip, '_ptr', recording_ptr)
    with torch.no_grad():
        g = EvalGraphs(model, x)
    monkeypatch.setattr(hip, '_ptr', ptr)
    assert len(seen) > 10
    gc.collect()
    torch.cuda.synchronize(dev)
    pool = tuple(g.graph_a.pool())
    segments = [(s['address'], s['address'] + s['total_size']) for s in torch.cuda.memory_snapshot()
                if tuple(s['segment_pool_id']) == pool]
    assert segments, 'no segment of the graphs\' private pool'
    dangling = [(addr, shape) for ref, addr, shape in seen
                if ref() is None and not any(lo <= addr < hi for lo, hi in segments)]
    assert not dangling, 'captured kernels read / write freed blocks outside the graph pool: {}'.format(dangling)


# ---- 2. the caching allocator hands every free small block out between capture and replay

def test_graphed_forward_survives_allocator_churn(S, dev, bench_mod):
    model = bench_mod.build_model(dev)
    xs = [bench_mod.synthetic_batch(1, dev, seed=s) for s in (6, 7)]
    ref = cold_outputs(model, lambda seed: bench_mod.build_model(dev, seed=seed), xs)
    with torch.no_grad():
        model(xs[0])
        assert model._eval_graphs_for(xs[0]) is not None
        torch.cuda.synchronize(dev)
        st = torch.cuda.memory_stats(dev)
        free = st['reserved_bytes.small_pool.current'] - st['allocated_bytes.small_pool.current']
        # 512 B is the small pool's granularity: blocks of it take every free small block whatever its size, none of them
        # splits a larger block for a later allocation.  Finite sentinels: a stale read gives wrong values, not a fault
        n = min(free // 512, 1 << 17)
        keep = [torch.full((128,), 1e4, device=dev) for _ in range(n)]
        got = [model(x) for x in xs]
        assert model._eval_graphs_for(xs[1]) is not None
        del keep
    for i, (a, b) in enumerate(zip(got, ref)):
        _assert_equal(a, b, 'image {} after {} small allocations'.format(i, n))


# ---- 3. inference mode (evaluate) and no_grad calls alternate

def _labelled_loader(x, logits, bs):
    labels = logits.float().argmax(1).cpu()
    labels[::3] = (labels[::3] + 1) % logits.shape[1]
    return torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x.cpu(), labels), batch_size=bs)


def _alternate_evaluate(S, model, build, x, bs, dev, exact, analyzers=False):
    """evaluate() -> model(x) under no_grad -> evaluate(), and model(x) under no_grad -> evaluate() -> model(x) under no_grad:
    the no_grad outputs equal the cold model's, both evaluate() runs count the same hits (and log the same data sizes)."""
    from sc2bench_amd import evaluation
    check = _assert_equal if exact else _assert_close
    xs = [x[i:i + bs] for i in range(0, len(x), bs)]      # (bs 1: the batches the graphs replay)
    ref = torch.cat(cold_outputs(model, build, xs))
    loader = _labelled_loader(x, ref, bs)
    want = 100.0 * (len(x) - len(range(0, len(x), 3))) / len(x)
    if analyzers:
        model.analyzes_after_compress = True
        model.analyzers = [S.FileSizeAnalyzer(unit='KB')]

    def run_eval():
        model.clear_analysis()
        r = evaluation.evaluate(model, loader, dev)
        assert r['samples'] == len(x)
        if exact:
            assert abs(r['acc1'] - want) < 1e-4, (r['acc1'], want)
        return r['acc1'], r['acc5'], r['analysis']

    def run_no_grad(what):
        with torch.no_grad():
            check(torch.cat([model(b) for b in xs]), ref, what)

    first = run_eval()                       # (bs 1: the graphs are captured here, under inference mode)
    run_no_grad('no_grad after evaluate')
    assert run_eval() == first
    run_no_grad('no_grad after two evaluate runs')
    if analyzers:
        assert first[2] and first[2][0]['count'] == len(x)
    return first


def _fp_builder(bench_mod, dev):
    return lambda seed: bench_mod.build_model(dev, seed=seed)


def test_fp_classifier_bs1_graphs_alternate_modes(S, dev, bench_mod):
    x = bench_mod.synthetic_batch(4, dev, seed=8)
    model = bench_mod.build_model(dev)
    _alternate_evaluate(S, model, _fp_builder(bench_mod, dev), x, 1, dev, exact=True, analyzers=True)
    with torch.no_grad():       # (the last evaluate() captured them: a capture that fails under inference mode falls back silently)
        assert model._eval_graphs_for(x[0:1]) is not None, model.__dict__.get('_eval_graphs_error')
        assert model.__dict__.get('_eval_graphs_error') is None, model.__dict__.get('_eval_graphs_error')
    # and the other order: the graphs captured under no_grad first
    model = bench_mod.build_model(dev)
    ref = cold_outputs(model, _fp_builder(bench_mod, dev), [x[i:i + 1] for i in range(len(x))])
    with torch.no_grad():
        _assert_equal(torch.cat([model(x[i:i + 1]) for i in range(len(x))]), torch.cat(ref), 'no_grad first')
    _alternate_evaluate(S, model, _fp_builder(bench_mod, dev), x, 1, dev, exact=True, analyzers=True)


def test_fp_classifier_pipelined_alternates_modes(S, dev, bench_mod):
    x = bench_mod.synthetic_batch(16, dev, seed=9)
    _alternate_evaluate(S, bench_mod.build_model(dev), _fp_builder(bench_mod, dev), x, 8, dev, exact=True)


def test_mshp_classifier_alternates_modes(S, dev, bench_mod):
    def build(seed):
        torch.manual_seed(seed)
        return bench_mod.build_workload('mshp224', dev, 4)[0]
    x = bench_mod.synthetic_batch(4, dev, seed=10)
    _alternate_evaluate(S, build(0), build, x, 2, dev, exact=True)


def _input_classifier(S, name, quality, dev, seed):
    from sc2bench_amd import transforms as T
    from sc2bench_amd.resnet import resnet50
    torch.manual_seed(seed)
    codec = S.COMPRESSION_MODEL_FUNC_DICT[name](quality=quality)
    clf = resnet50(num_classes=10).eval()
    model = S.NeuralInputCompressionClassifier(clf, pre_transform=T.AdaptivePad(fill=0, factor=64), compression_model=codec,
                                               post_transform=T.Compose([T.CenterCrop([64, 64])]), analysis_config={})
    model.eval().to(dev)
    codec.update()
    model.set_compute_dtype('bf16')
    return model


@pytest.mark.parametrize('name', ['bmshj2018_factorized', 'bmshj2018_hyperprior', 'mbt2018'])
def test_input_compression_classifiers_alternate_modes(S, dev, name):
    def build(seed):
        return _input_classifier(S, name, 1, dev, seed)
    x = torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(12)).to(dev)
    _alternate_evaluate(S, build(0), build, x, 2, dev, exact=False)


def _dense_builder(bench_mod, name, n, dev):
    def build(seed):
        torch.manual_seed(seed)
        return bench_mod.build_workload(name, dev, n)[0]
    return build


@pytest.mark.parametrize('name,n,hw', [('seg513', 1, (257, 257)), ('det800x1216', 1, (320, 416))])
def test_dense_models_alternate_modes(S, dev, bench_mod, name, n, hw):
    """inference mode -> no_grad -> inference mode and the reverse, on the dense models and their feature-extraction bodies"""
    build = _dense_builder(bench_mod, name, n, dev)
    x = torch.rand(n, 3, hw[0], hw[1], generator=torch.Generator().manual_seed(13)).to(dev)
    for first, second in ((torch.inference_mode, torch.no_grad), (torch.no_grad, torch.inference_mode)):
        model = build(0)
        (ref,), (ref_body,) = cold_outputs(model, build, [x], body=True)
        for mode in (first, second, first, second):
            with mode():
                _assert_close(model(x), ref, '{} under {}'.format(name, mode.__name__))
                _assert_equal(model._body()(x), ref_body, '{} body under {}'.format(name, mode.__name__))


# ---- 4. parameters replaced rather than written

def _mutations(dev):
    def fc_data(m):
        m.fc.weight.data = _like(m.fc.weight, m.fc.weight.detach().roll(1, 0))

    def new_parameter(m):
        w = m.layer4[0].conv2.weight
        m.layer4[0].conv2.weight = nn.Parameter(_like(w, w.detach().roll(1, 0)))

    def layer_assign(m):
        sd = {k: (_like(v, v.roll(1, 0)) if k.endswith('conv2.weight') else v.clone()) for k, v in m.layer3.state_dict().items()}
        m.layer3.load_state_dict(sd, assign=True)

    def root_assign(m):
        sd = copy.deepcopy(m.state_dict())
        w = sd['layer2.0.conv1.weight']
        sd['layer2.0.conv1.weight'] = _like(w, -w)
        m.load_state_dict(sd, assign=True)

    def encoder_data(m):
        w = m.bottleneck_layer.encoder[4].weight
        w.data = _like(w, w.detach() * 0.8)

    def quantiles_data(m):
        q = m.bottleneck_layer.entropy_bottleneck.quantiles
        v = q.detach().clone()
        v[:, :, 1] += 0.5
        q.data = v

    def quantiles_add(m):
        with torch.no_grad():
            m.bottleneck_layer.entropy_bottleneck.quantiles.add_(0.5)

    def cpu_round_trip(m):
        m.cpu()
        with torch.no_grad():
            m.fc.bias.add_(1.0)
        m.to(dev)
        torch.cuda.synchronize(dev)

    return {f.__name__: f for f in (fc_data, new_parameter, layer_assign, root_assign, encoder_data, quantiles_data, quantiles_add,
                                    cpu_round_trip)}


@pytest.mark.parametrize('case', ['fc_data', 'new_parameter', 'layer_assign', 'root_assign', 'encoder_data', 'quantiles_data',
                                  'quantiles_add', 'cpu_round_trip'])
def test_replaced_parameters_reach_graphs_and_eager_head(S, dev, bench_mod, case):
    """bs 1 (graphed) and bs 2 (eager HIP head), run before and after the change: equal to the cold model with the new weights.
    The quantiles cases change no CDF table (no update()): the eager path is the specification -- the medians follow the quantiles."""
    model = bench_mod.build_model(dev)
    x1, x2 = bench_mod.synthetic_batch(1, dev, seed=14), bench_mod.synthetic_batch(2, dev, seed=15)
    with torch.no_grad():
        before = [model(x1), model(x2)]
        assert model._eval_graphs_for(x1) is not None
    _mutations(dev)[case](model)
    ref = cold_outputs(model, _fp_builder(bench_mod, dev), [x1, x2])
    with torch.no_grad():
        got = [model(x1), model(x2)]
        assert model._eval_graphs_for(x1) is not None, model.__dict__.get('_eval_graphs_error')
    assert not torch.equal(ref[0], before[0]), 'the change does not move the output: the case tests nothing'
    _assert_equal(got[0], ref[0], '{}: bs 1 (graphs)'.format(case))
    _assert_equal(got[1], ref[1], '{}: bs 2 (eager)'.format(case))


@pytest.mark.parametrize('name,n,hw', [('seg513', 1, (257, 257)), ('det800x1216', 1, (320, 416))])
def test_replaced_parameters_reach_dense_models(S, dev, bench_mod, name, n, hw):
    build = _dense_builder(bench_mod, name, n, dev)
    model = build(0)
    x = torch.rand(n, 3, hw[0], hw[1], generator=torch.Generator().manual_seed(16)).to(dev)
    body = model._body()
    with torch.no_grad():
        before = model(x)
    w = body.layer3[0].conv2.weight
    w.data = _like(w, w.detach().roll(1, 0))
    if name == 'det800x1216':
        conv = model.fpn.inner_blocks[1][0]
        conv.weight = nn.Parameter(_like(conv.weight, -conv.weight.detach()))
    (ref,), (ref_body,) = cold_outputs(model, build, [x], body=True)
    with torch.no_grad():
        got, got_body = model(x), body(x)
    _assert_close(got, ref, name)
    _assert_equal(got_body, ref_body, name + ' body')
    assert not all(torch.equal(a, b) for a, b in zip(ref.values(), before.values()))


# ---- 6. several captured input shapes alive at once, and one beyond the limit

def test_several_captured_shapes_interleaved(S, dev, bench_mod):
    model = bench_mod.build_model(dev)
    g = torch.Generator().manual_seed(17)
    shapes = [(224, 224), (160, 192), (192, 160), (128, 128), (96, 128), (256, 224)]
    xs = [(torch.rand(1, 3, h, w, generator=g) * 2 - 1).to(dev) for h, w in shapes]
    ref = cold_outputs(model, _fp_builder(bench_mod, dev), xs)
    with torch.no_grad():
        for order in ([0, 1, 0, 1], [2, 3, 4, 0, 5, 1, 5, 3]):
            for i in order:
                _assert_equal(model(xs[i]), ref[i], 'shape {}'.format(shapes[i]))
        graphed = [model._eval_graphs_for(x) is not None for x in xs]
    assert graphed[:5] == [True] * 5 and not graphed[5], graphed     # (max_shapes = 4: the sixth shape runs eagerly)
