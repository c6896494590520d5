"""GPU timing of the Pillow-exact resampler (car_resize).  Reported, not gated.  Not a test.

Shapes: 1024 x 1024 x 3 -> 512 x 512 BICUBIC at B = 1 and B = 16, and 2048 x 1536 x 3 -> 512 x 384 LANCZOS at B = 1 (heights first).  Per shape: 5 warm-up
calls, then `--repeats` calls through the C ABI on preallocated tensors, timed one by one with device events on the caller's stream; median, min and
max.  Bytes moved are the algorithm's: the source rows the vertical bounds touch, the uint8 intermediate written and read once, the result written.
The fraction of HBM bandwidth is those bytes over the median time against 8.0 TB/s.  `ms_gather_form` is the same call in the development build with
CAR_RESIZE_NO_LDS set: the horizontal pass as a byte gather from global memory instead of the LDS-staged form the library picks for these shapes.
The result of the first call is compared with Pillow's when Pillow imports, and Pillow's own time for the same resizes on the host (one image after the other, median of 5) is recorded next to it.
usage: resize_time.py [--repeats 21] [--out-dir profiles]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [  # B, H, W, Ho, Wo, filter name
    (1, 1024, 1024, 512, 512, "bicubic"),
    (16, 1024, 1024, 512, 512, "bicubic"),
    (1, 2048, 1536, 512, 384, "lanczos"),
]
HBM_PEAK = 8.0e12


def main(a):
    import numpy as np
    import torch
    from controlar_amd import _lib as L, config as Cfg
    from controlar_amd.engine import Engine, RESAMPLE_CODES
    try:
        from PIL import Image
    except ImportError:
        Image = None
    eng = Engine(Cfg.tiny_t2i(), "bf16")
    dev = Engine(Cfg.tiny_t2i(), "bf16", dev=True)
    lines = []
    for B, H, W, Ho, Wo, fname in SHAPES:
        f = RESAMPLE_CODES[fname]
        x = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
        xg = x.cuda()
        out = torch.empty(B, Ho, Wo, 3, dtype=torch.uint8, device="cuda")
        ctrl = torch.empty(B, 3, Ho, Wo, dtype=eng.dtype, device="cuda")

        def call(with_control, eng=eng):
            st = C.c_void_p(int(torch.cuda.current_stream().cuda_stream))
            rc = eng.lib.car_resize(eng._h, C.c_void_p(xg.data_ptr()), B, H, W, 3, Ho, Wo, f, None, C.c_void_p(out.data_ptr()),
                                    C.c_void_p(ctrl.data_ptr() if with_control else 0), C.c_void_p(0), 0, st)
            assert rc == 0, eng.lib.car_last_error(eng._h)

        def timed(with_control, eng=eng):
            go = lambda wc: call(wc, eng)
            for _ in range(5):
                go(with_control)
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); go(with_control); e1.record(); e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            return statistics.median(ms), min(ms), max(ms)

        # the vertical bounds decide which source rows the horizontal pass makes
        ks = C.c_int32(0)
        cap = Ho * (2 * int(np.ceil(3 * max(H / Ho, 1.0))) + 1)
        kk, bounds = np.zeros(cap, np.int32), np.zeros(Ho * 2, np.int32)
        assert L.load().car_debug_resample_coeffs(H, 0.0, float(H), Ho, f, C.byref(ks), C.c_void_p(kk.ctypes.data), C.c_void_p(bounds.ctypes.data), cap) == 0
        b2 = bounds.reshape(Ho, 2)
        nrows = int((b2[:, 0] + b2[:, 1]).max() - b2[:, 0].min())
        pitch = (Wo * 3 + 3) // 4 * 4
        nbytes = B * (nrows * W * 3 + 2 * nrows * pitch + Ho * Wo * 3)
        med, lo, hi = timed(False)
        rec = dict(stage="car_resize", B=B, H=H, W=W, Ho=Ho, Wo=Wo, filter=fname, ksize_v=int(ks.value), ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                   bytes=nbytes, gb_per_s=round(nbytes / med / 1e6, 1), hbm_fraction_of_8TBs=round(nbytes / (med * 1e-3) / HBM_PEAK, 4), kernel_form="two-pass, LDS-staged horizontal")
        os.environ["CAR_RESIZE_NO_LDS"] = "1"
        try:
            rec["ms_gather_form"] = round(timed(False, dev)[0], 4)
        finally:
            del os.environ["CAR_RESIZE_NO_LDS"]
        medc, loc, hic = timed(True)
        rec.update(ms_with_control=round(medc, 4), bytes_with_control=nbytes + B * 3 * Ho * Wo * ctrl.element_size())
        if Image is not None:
            imgs = [Image.fromarray(x[i].numpy()) for i in range(B)]
            call(False)
            torch.cuda.synchronize()
            rec["equals_pillow"] = bool(all(np.array_equal(out[i].cpu().numpy(), np.asarray(imgs[i].resize((Wo, Ho), f))) for i in range(B)))
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                for im in imgs:
                    im.resize((Wo, Ho), f)
                ts.append((time.perf_counter() - t0) * 1e3)
            rec["pillow_host_ms"] = round(statistics.median(ts), 3)
        else:
            rec["pillow_host_ms"] = None
        print("RESIZE_TIME " + json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    eng.close()
    dev.close()
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "resize_time.jsonl"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    main(ap.parse_args())
