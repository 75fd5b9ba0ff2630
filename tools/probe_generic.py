#!/usr/bin/env python3
"""k_generic (csic_process_device under CSIC_TUNE_FORCE_GENERIC) timed with device events; one library per process (CSIC_LIB)."""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import csic_amd as csic
N = csic._native
OUT = sys.argv[1]
REPS, CALLS, ROT = 9, 12, 3
CSQ, SCQ = (3, 1, 2), (1, 3, 2)
rows = []
for (name, W, H, a, b, f, op, infmt) in (("4k_420_f2_cfirst", 3840, 2160, 2, 0, 2, CSQ, 0), ("4k_420_f2_sfirst", 3840, 2160, 2, 0, 2, SCQ, 0),
                                         ("4k_420_f1", 3840, 2160, 2, 0, 1, CSQ, 0), ("1001_411_f4_sfirst", 1001, 1001, 1, 1, 4, SCQ, 0),
                                         ("4k_420_f2_sfirst_yccin", 3840, 2160, 2, 0, 2, SCQ, 1)):
    bufs = [torch.randint(0, 1 << 24, (W * H,), dtype=torch.int32, device="cuda:0") for _ in range(ROT)]
    with csic.Plan(csic.make_c_params(W, H, a, b, 6, 5, 5, f, op, in_format=infmt), 0) as pl:
        pl.tune(N.TUNE_FORCE_GENERIC, 1)
        assert pl.kernel_name.startswith("k_generic"), pl.kernel_name
        out = pl.process_device(bufs[0])
        us = []
        for rep in range(REPS + 1):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for i in range(CALLS):
                pl.process_device(bufs[i % ROT], out)
            e.record(); e.synchronize()
            if rep: us.append(s.elapsed_time(e) * 1e3 / CALLS)
        r = {"case": name, "kernel": pl.kernel_name, "us": round(statistics.median(us), 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2)}
        print(json.dumps(r), flush=True); rows.append(r)
    del bufs
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as fh:
    for r in rows: fh.write(json.dumps(r) + "\n")
