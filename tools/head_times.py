"""Per-launch timing of the fused inference head (layer2..fc) at bs 256: where the 53 launches spend their time.

    python tools/head_times.py                  one table, the policy in force
    python tools/head_times.py --w8-ab [R]      the 1x1 layers conv1x1_w8.hip supports under conv1x1_w8 = '0' and 'all', alternating in
                                                this one process, R rounds (default 5): per (cin, cout, stride) tuple the summed launch
                                                times of every round and whether the new kernel won EVERY round -- the rule by which a
                                                tuple enters head._W8_TABLE
"""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench as B
from sc2bench_amd import hip
from tools import env_policy  # (the SC2_* variables of the A/B scripts -> the dispatch policy)
env_policy.apply()
dev = torch.device('cuda:0')
m = B.build_model(dev)
N = 256
x = torch.randn(N, 56, 56, 256, device=dev).to(torch.bfloat16).permute(0, 3, 1, 2)
if '--w8-ab' in sys.argv:
    i = sys.argv.index('--w8-ab')
    rounds = int(sys.argv[i + 1]) if len(sys.argv) > i + 1 else 5
    with torch.no_grad():
        m.head(x)
    torch.cuda.synchronize()
    tuples = {}    # tag -> (cin, cout, stride) of the layers the kernel supports
    for blk in m._hip_head.blocks:
        for c in blk:
            if c is not None and getattr(c, 'w8_ok', False):
                tuples[c.tag] = (c.cin, c.cout, c.stride[0])
    keys = sorted(set(tuples.values()))
    table = {k: [] for k in keys}
    head_ms = []
    before = hip.host_policy.conv1x1_w8
    with torch.no_grad():
        for rnd in range(rounds):
            row, hrow = {}, []
            for mode in ('0', 'all'):
                hip.configure(conv1x1_w8=mode)
                for _ in range(3): m.head(x)
                torch.cuda.synchronize()
                with hip.KernelTimer() as t:
                    for _ in range(5): m.head(x)
                    torch.cuda.synchronize()
                summ = t.summary()
                hrow.append(sum(ms for _, ms in summ.values()))
                for tag, k in tuples.items():
                    if tag in summ:
                        row.setdefault(k, [0.0, 0.0, 0])
                        row[k][0 if mode == '0' else 1] += summ[tag][1]
                        row[k][2] += mode == '0'
            for k in keys:
                table[k].append(row.get(k, [float('nan'), float('nan'), 0]))
            head_ms.append(hrow)
    hip.configure(conv1x1_w8=before)
    print('{:<22} {:>3}  {}   (ms per round: before -> w8, summed over the tuple\'s launches)'.format('(cin, cout, stride)', 'n', 'rounds'))
    for k in keys:
        rs = table[k]
        wins = all(r[1] < r[0] for r in rs)
        print('{:<22} {:>3}  {}  {}'.format(str(k), rs[0][2], '  '.join('{:.4f}->{:.4f}'.format(r[0], r[1]) for r in rs),
                                            'W8 FASTER IN EVERY ROUND' if wins else 'stays'))
    print('sum of the head\'s launches per round, before -> all:', '  '.join('{:.3f}->{:.3f}'.format(a, b) for a, b in head_ms))
    sys.exit(0)
with torch.no_grad():
    for _ in range(3): m.head(x)
    torch.cuda.synchronize()
    with hip.KernelTimer() as t:
        for _ in range(5): m.head(x)
        torch.cuda.synchronize()
hd = m._hip_head
rows = []
shapes = {}
H = 56
for (c1, c2, c3, ds) in hd.blocks:
    pass
tot = 0
for tag, (cnt, ms) in sorted(t.summary().items(), key=lambda kv: -kv[1][1]):
    tot += ms
    print('{:<16} {:7.3f} ms'.format(tag, ms))
print('total', tot)
