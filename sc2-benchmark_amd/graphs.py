"""HIP-graph replay of the updated evaluation forward at small batch sizes.

The reference measures data size -- and evaluates -- at test batch size 1 (script/task/image_classification.py:106-145,
README.md:100-108): `output = model(image)` = encode -> bytes -> analyzers -> decode -> layer2..fc, one image after the other.  On
the GPU that forward is ~45 launches of a few microseconds each around a host range coder (entropy.py: one serial rANS stream
per image is a CPU core's job), and at that size what the device spends is mostly the distance BETWEEN launches: the Python
wrapper and the runtime's launch path per kernel, ~0.3 ms of a 1.95 ms forward (tools/bs1_prof.py).  `EvalGraphs` captures the
two device halves once per input shape --

    A  x  -> encoder (conv0 + GDN, conv2 + GDN, conv4 with the quantiser in its epilogue) -> int32 symbols
    B  int32 symbols -> dequantise -> decoder -> layer2 .. fc -> output

-- and replays them around the same host coder calls: the same kernels with the same arguments in the same order (outputs are
bit-identical to the eager forward, tests/test_gpu_graphs.py), no re-exec, no second process.  The byte strings, the
{'strings', 'shape'} object the analyzers see and the status checks are the eager path's.

A captured graph bakes in device addresses: of the packed weights (re-packed when a parameter's storage or version changes), of
the CDF tables, of the median vector and of its static input / output buffers -- every one of them owned by the graph or the model
for as long as the graph lives.  The version and address of every parameter and buffer are compared per call (`signature`); a
parameter, buffer or submodule registered anywhere (`m.weight = nn.Parameter(..)`, `load_state_dict(assign=True)`) makes the next
call walk the module tree again; and the model drops its graphs when its storage is re-homed or its mode changes (`invalidate`);
the next call captures again.  A graph is captured outside inference mode whatever the caller's, so that evaluate()'s
torch.inference_mode and a plain no_grad caller can take turns on it.  Persistent kernels take their work counters from a region
of their own when captured (csrc/sc2_common.h: sc2_counter_ring::launch_slot), so a replay never shares a counter with an eager
launch on another stream.
"""
import numpy as np
import torch
from torch import nn

from . import hip

__all__ = ['EvalGraphs', 'graphs_for']


# bumped whenever any module of the process registers a parameter, buffer or submodule (assignment, register_*, load_state_dict
# with assign=True): the tensor list kept with a model's graphs may then be stale
_registrations = [0]


def _registered(module, name, value):
    _registrations[0] += 1


for _hook in (nn.modules.module.register_module_parameter_registration_hook,
              nn.modules.module.register_module_buffer_registration_hook,
              nn.modules.module.register_module_module_registration_hook):
    _hook(_registered)


def _tensors(model):
    return list(model.parameters()) + list(model.buffers())


def signature(tensors):
    """what a captured graph depends on besides its input: the version and the address of every tensor of the model (`p.data = t`
    keeps the version; walking the module tree for the tensors costs 0.4 ms, so the list is kept with the graphs and taken again
    only after a registration).  Re-homed storage (`.to()`, `load_state_dict`, `update()`, a change of mode or precision) drops
    the graphs through `invalidate`."""
    return hash(tuple((t._version, t.data_ptr()) for t in tensors))


def invalidate(model):
    model.__dict__.pop('_eval_graphs', None)


class EvalGraphs(object):
    """Graphs A and B of ONE input shape of a `SplittableResNet`-like model (attributes: bottleneck_layer with
    analysis / entropy_bottleneck, decode_head)."""

    def __init__(self, model, x):
        # (outside inference mode whatever the caller's: a graph captured under evaluate()'s torch.inference_mode is replayed by a
        #  later call under plain no_grad, which writes x_static / sym_in in place)
        with torch.inference_mode(False), torch.no_grad():
            self._capture(model, x)

    def _capture(self, model, x):
        bl = model.bottleneck_layer
        eb = bl.entropy_bottleneck
        dev = x.device
        self.shape_key = (tuple(x.shape), x.dtype)
        self.x_static = x.detach().clone()
        # graph B reads the medians from this address on every replay: the graph owns the vector
        self.medians = medians = eb._median_vector()
        # warm-up on a side stream (weights packed, LDS attributes set, work counters allocated, caching-allocator pools
        # filled): a first launch of a persistent kernel cannot be captured (hipMalloc), and torch asks for it anyway
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(2):
                sym = bl.analysis(self.x_static, symbols_for=eb)
                y_hat = hip.eb_dequantize(sym, medians, want_f32=False, want_nhwc=True)[1]
                model.decode_head(y_hat)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.latent_shape = tuple(sym.shape[-2:])
        self.graph_a = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph_a):
            self.sym_out = bl.analysis(self.x_static, symbols_for=eb)
        self.sym_in = torch.zeros_like(self.sym_out)
        self.graph_b = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph_b, pool=self.graph_a.pool()):
            y_hat = hip.eb_dequantize(self.sym_in, medians, want_f32=False, want_nhwc=True)[1]
            self.out = model.decode_head(y_hat)
        # pinned staging for the two host transfers (symbols out, decoded symbols in)
        self.sym_host = torch.empty(self.sym_out.shape, dtype=torch.int32, pin_memory=True)
        self.dec_host = torch.empty(self.sym_out.shape, dtype=torch.int32, pin_memory=True)

    def symbols(self, x):
        """graph A on `x`: -> int32 numpy [N, C*h*w] view of the pinned staging buffer (valid until the next call)."""
        self.x_static.copy_(x)
        self.graph_a.replay()
        self.sym_host.copy_(self.sym_out, non_blocking=True)
        torch.cuda.current_stream(x.device).synchronize()
        return self.sym_host.view(self.sym_host.shape[0], -1).numpy()

    def decode_head(self, symbols_host):
        """decoded int32 symbols (numpy [N, C*h*w]) -> the model's output (a clone the caller owns)."""
        np.copyto(self.dec_host.view(self.dec_host.shape[0], -1).numpy(), symbols_host)
        self.sym_in.copy_(self.dec_host, non_blocking=True)
        self.graph_b.replay()
        out = self.out
        return out.clone() if isinstance(out, torch.Tensor) else type(out)((k, v.clone()) for k, v in out.items())


def graphs_for(model, x, max_shapes=4):
    """The EvalGraphs of (model, x's shape), captured on first use; None when graphs do not apply or capture fails (the caller
    runs the eager forward; the reason is kept in `model._eval_graphs_error`)."""
    cache = model.__dict__.setdefault('_eval_graphs', {})
    if cache.get('registrations') != _registrations[0]:
        cache['tensors'], cache['registrations'] = _tensors(model), _registrations[0]
    sig = signature(cache['tensors'])
    if cache.get('sig') != sig:
        tensors, registrations = cache['tensors'], cache['registrations']
        cache.clear()
        cache['tensors'], cache['registrations'], cache['sig'] = tensors, registrations, sig
    key = (tuple(x.shape), x.dtype, x.device)
    g = cache.get(key)
    if g is None and key not in cache:
        if len(cache) > max_shapes + 3:      # a loader of ever-changing shapes: stop capturing, run eagerly
            return None
        try:
            g = EvalGraphs(model, x)
            # (capturing allocates packed weights on first use: take the signature again so that the next call matches)
            if cache['registrations'] != _registrations[0]:
                cache['tensors'], cache['registrations'] = _tensors(model), _registrations[0]
            cache['sig'] = signature(cache['tensors'])
        except Exception as e:      # noqa: BLE001 -- a capture that fails must leave the eager path usable
            model.__dict__['_eval_graphs_error'] = repr(e)
            torch.cuda.synchronize(x.device)
            g = None
        cache[key] = g
    return g
