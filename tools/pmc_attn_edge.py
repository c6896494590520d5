"""HBM fetch of the bf16 decode attention per decode step, from one `rocprofv3 --pmc FETCH_SIZE` pass over tools/pmc_workload.py, against the row-count
formula of its edge blocks (profiles/attn_trim_ab.txt).

usage: pmc_attn_edge.py <counter_collection.csv> <B> <first_pos> <steps>
The workload runs eagerly (CAR_NO_GRAPH): the dec_attn2 dispatches come in step order, n_layer x chains per step.  Per step the measured mean per launch
(FETCH_SIZE KiB x 2: the gfx950 wide-read correction of tools/pmc_decode.py) is printed beside three predictions for the benchmark's seeded prompts
(synth.text_embeddings: jmin = 120 - valid length), in bytes per launch = rows x 128 B x heads x sequences of a chain, K and V:
  exact    rows in [jmin, pos]                                               (what decode_algo_bytes counts)
  blocks   whole 32-position blocks jmin>>5 .. pos>>5                        (every lane of an edge block loads)
  trimmed  K: 8 x octets that meet [jmin, pos]; V: 8 x (block, lane group) pairs with a quartet in range"""
import csv, os, sys
from collections import defaultdict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
path, B, pos0, steps = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
from controlar_amd import config as C, synth
cfg = C.xl_t2i(1024)
H, T = cfg.gpt.n_head, cfg.gpt.cls_token_num
_, mask = synth.text_embeddings(B, T, cfg.gpt.caption_dim)
jmins = [int((mask[i] != 0).nonzero()[0]) for i in range(B)]


def rows(jmin, pos):
    exact = pos - jmin + 1
    blocks = 32 * ((pos >> 5) - (jmin >> 5) + 1)
    k = 8 * len({t >> 3 for t in range(jmin, pos + 1)})
    v = 8 * len({(t >> 5, (t & 15) >> 2) for t in range(jmin, pos + 1)})
    return exact, blocks, k, v


acc = defaultdict(float)      # a dispatch may report one row per counter instance: summed
with open(path) as f:
    for r in csv.DictReader(f):
        if r["Counter_Name"] == "FETCH_SIZE" and "dec_attn2_kernel" in r["Kernel_Name"]:
            acc[int(r["Dispatch_Id"])] += float(r["Counter_Value"])
disp = sorted(acc.items())
per = len(disp) // steps
print(f"{len(disp)} dec_attn2 dispatches, {per} per step ({B} sequences, {H} heads); bytes per launch, mean over a step's launches")
chains = 2 if B >= 192 else 1
prev = None
for s in range(steps):
    pos = pos0 + s
    meas = sum(v for _, v in disp[s * per:(s + 1) * per]) / per * 1024.0 * 2.0
    tot = defaultdict(float)
    for j in jmins:
        e, b, k, v = rows(j, pos)
        tot["exact"] += 2 * e; tot["blocks"] += 2 * b; tot["trimmed"] += k + v
    pred = {n: t * 128.0 * H / chains for n, t in tot.items()}
    line = f"pos {pos} (pos & 31 = {pos & 31:2d}): measured {meas / 1e6:9.2f} MB   exact {pred['exact'] / 1e6:9.2f}  blocks {pred['blocks'] / 1e6:9.2f}  trimmed {pred['trimmed'] / 1e6:9.2f}" \
           f"   measured / exact {meas / pred['exact']:.4f}  / blocks {meas / pred['blocks']:.4f}  / trimmed {meas / pred['trimmed']:.4f}"
    if prev is not None:
        line += f"   step from previous: measured {(meas - prev[0]) / 1e6:+.2f} MB, blocks {(pred['blocks'] - prev[1]) / 1e6:+.2f}, trimmed {(pred['trimmed'] - prev[2]) / 1e6:+.2f}"
    prev = (meas, pred["blocks"], pred["trimmed"])
    print(line)
