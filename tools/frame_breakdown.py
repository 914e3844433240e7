"""Where does one 1080p P picture go?  enqueue (Python) / GPU / D2H / rANS."""
import os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vcm_ts_amd.dmc import DMC
from vcm_ts_amd.intra import IntraNoAR
from vcm_ts_amd.pipeline import pad_frame
from bench import synth_sequence
prec = sys.argv[1] if len(sys.argv) > 1 else "fp16x3"
dev = torch.device("cuda:0")
i_net, p_net = IntraNoAR(precision=prec).to(dev).eval(), DMC(precision=prec).to(dev).eval()
i_net.update(); p_net.update()
seq = [pad_frame(f) for f in synth_sequence(dev, 6, 1080, 1920, 0)]
dpb = {"ref_frame": i_net.compress(seq[0], 1.0)["x_hat"], "ref_feature": None, "ref_y": None, "ref_mv_y": None}
dpb = p_net.compress(seq[1], dpb, 1.0, 1.0)["dpb"]
torch.cuda.synchronize()
for t in (2, 3, 4):
    t0 = time.perf_counter()
    o = p_net._run(seq[t], dpb, 1.0, 1.0, "compress")
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    pending = p_net._stage_symbols(p_net._planes(o))  # the product's staging: six planes into one pinned buffer
    pending.event.synchronize()
    t3 = time.perf_counter()
    ec = p_net.entropy_coder; ec.reset_encoder()
    pending.encode_element(0)
    t4 = time.perf_counter()
    bs = ec.flush_encoder()
    t5 = time.perf_counter()
    pending._streams = [bs]  # retired: its staging slot may be reused
    dpb = p_net._dpb_out(o)
    print(f"P{t}: enqueue {1e3*(t1-t0):.1f} ms | gpu drain {1e3*(t2-t1):.1f} | D2H(pinned, async + wait) {1e3*(t3-t2):.1f} | encode_with_indexes {1e3*(t4-t3):.1f} | flush {1e3*(t5-t4):.1f} | bytes {len(bs)} | launches {p_net.engine().calls}")
