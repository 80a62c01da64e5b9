#!/usr/bin/env python3
"""The multi-prime mod-down kernels at every compiled width, for a kernel trace or tools/lib_ab.sh:
CKKS N = 2^15, eight 50-bit ciphertext primes and P = 2, 4, 8, 9 special primes (k_moddown_extended<2 / 4 / 8 / 16>,
k_moddown_multi_stage_one<the same>), 16 ciphertexts.  Per P: `reps` calls of hegpu_divide_round_lastq_extended (mode 1)
and of the method II relinearize, device-event times and a checksum of both outputs.  usage: moddown_ab.py [reps]"""
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import heongpu_amd as hg  # noqa: E402
from helpers import synth_ct, synth_key  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
n, Q, batch = 1 << 15, 8, 16


def timed(f):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


for P in (2, 4, 8, 9):
    c = hg.Context.from_bit_sizes(hg.CKKS, n, [50] * Q, [50] * P, sec=hg.SEC_NONE)
    primes = [int(v) for v in c.table("modulus")]
    c.upload()
    Qp = Q + P
    src = hg.to_device(np.tile(synth_ct(primes, range(Qp), 2, n, 7), batch))
    ct = hg.to_device(np.tile(synth_ct(primes, range(Q), 3, n, 9), batch))
    key = hg.to_device(synth_key(primes, -(-Q // P), Qp, n, 3))
    out = torch.empty(batch * 2 * Q * n, dtype=torch.int64, device="cuda")
    ws = c.workspace(hg.OP_CKKS_RELIN, 0, batch)
    work = ct.clone()

    def extended():
        c.divide_round_lastq_extended(src, 2 * Qp * n, ct, 3 * Q * n, out, 2 * Q * n, 1, 0, batch)

    def relin():
        work.copy_(ct)
        c.ckks_relinearize_inplace(work, 3 * Q * n, key, 0, batch, ws)

    t_ext, t_relin = timed(extended), timed(relin)
    crc = zlib.crc32(hg.to_host(out).tobytes()), zlib.crc32(hg.to_host(work).tobytes())
    print("P=%d: moddown_extended %.1f us, relinearize (with its input copy) %.1f us, crc %08x %08x" % ((P, t_ext, t_relin) + crc),
          flush=True)
