"""Where the logit difference between the routing with and without conv1x1_w8.hip comes from (bs 256, the benchmark's batch).

The kernel reproduces conv1x1_win bit for bit; layers it takes from conv1x1_kres change their summation order (two K halves -> one
chain), i.e. some bf16 outputs round the other way, and later layers carry that on.  This tool shows it:
  1. per launch: conv1 of a layer3 block on conv1x1_kres, conv1x1_win and conv1x1_w8 -- share of outputs that differ and by how much;
  2. per tuple: the logits with ONE tuple of head._W8_TABLE switched in, with the former-kres tuples, the former-win tuples, the table;
  3. control: the same former-kres tuples sent to the EXISTING conv1x1_win kernel instead (a head rebuilt with a wider _win1_policy,
     conv1x1_w8 off) -- must equal the table's logits bit for bit.
    python tools/w8_logit_attribution.py"""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench as B
from sc2bench_amd import hip, head as H

dev = torch.device('cuda:0')
m = B.build_model(dev)
x = B.synthetic_batch(256, dev)
KRES = tuple(t for t in H._W8_TABLE if t[0] == 1024)
WIN = tuple(t for t in H._W8_TABLE if t[0] != 1024)
TABLE = H._W8_TABLE


def stats(name, out, ref):
    d = (out.float() - ref.float()).abs()
    scale = ref.float().abs().max().item()
    same = int((out.float().argmax(1) == ref.float().argmax(1)).sum())
    q = torch.quantile(d.flatten()[:16000000].float(), torch.tensor([0.5, 0.99, 0.9999], device=d.device))
    print('{:<34} max {:.4f} ({:.3f} % of max|logit| {:.2f})  mean {:.5f}  median {:.5f}  p99 {:.4f}  p99.99 {:.4f}  differing {:.1f} %  argmax equal {} / {}'.format(
        name, d.max().item(), 100 * d.max().item() / scale, scale, d.mean().item(), q[0].item(), q[1].item(), q[2].item(),
        100.0 * (d > 0).float().mean().item(), same, out.shape[0]))


with torch.no_grad():
    # 1. one launch
    g = torch.Generator().manual_seed(1)
    xa = torch.randn(256, 14, 14, 1024, generator=g).to(torch.bfloat16).to(dev)
    w = (torch.randn(256, 1024, 1, 1, generator=g) / 32).to(dev)
    b = torch.randn(256, generator=g).to(dev)
    yk = hip.conv1x1_kres_fwd(xa, hip.pack_weight_fragments(w.reshape(256, 1024)), b, relu=True)
    yw = hip.conv1x1_win_fwd(xa, hip.pack_conv_win(w), b, relu=True)
    y8 = hip.conv1x1_w8_fwd(xa, hip.pack_conv_win(w), b, relu=True)
    ne = (yk != yw)
    steps = (yk.view(torch.int16).int() - yw.view(torch.int16).int()).abs()      # distance in bf16 steps (same sign: ReLU outputs)
    print('one launch, 1024 -> 256 at 50 176 pixels: conv1x1_w8 == conv1x1_win bit for bit: {};  conv1x1_kres differs from them in {:.2f} % of the '
          'outputs, by at most {} bf16 step(s)'.format(torch.equal(y8, yw), 100.0 * ne.float().mean().item(), int(steps.max().item())))
    # 2. logits per tuple
    sym, hw = m.stage_front(x)
    dec, _, _ = m.stage_coder(sym, hw, dequantized=True)
    hip.configure(conv1x1_w8='0')
    ref = m.stage_back(dec, hw).clone()
    assert torch.equal(m.stage_back(dec, hw), ref)
    hip.configure(conv1x1_w8='1')
    outs = {}
    for name, tab in [(str(t), (t,)) for t in TABLE] + [('former conv1x1_kres tuples', KRES), ('former conv1x1_win tuples', WIN), ('the table', TABLE)]:
        H._W8_TABLE = tab
        outs[name] = m.stage_back(dec, hw).clone()
        stats(name, outs[name], ref)
    H._W8_TABLE = TABLE
    # 3. control: the former-kres tuples on the existing conv1x1_win kernel
    hip.configure(conv1x1_w8='0')
    old = H._win1_policy
    H._win1_policy = lambda cin, cout, stride: old(cin, cout, stride) or (cin, cout, stride) in KRES
    m._hip_head = None
    ctl = m.stage_back(dec, hw).clone()
    H._win1_policy = old
    m._hip_head = None
    hip.configure(conv1x1_w8='1')
    stats('control: kres tuples -> conv1x1_win', ctl, ref)
    print('control logits equal the table\'s logits bit for bit:', torch.equal(ctl, outs['the table']))
