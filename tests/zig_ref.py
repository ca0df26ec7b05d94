"""Host pieces of the Gaussian DGP's draw contract that tests need to classify a replicate's normals:
Philox4x32-10 on numpy arrays, the ziggurat tables read from csrc/dcor_tables.h, and attempt 0's
fast-path value of each normal of a replicate."""
import os
import re

import numpy as np

SITE_DGP_A = 1
TABLES_H = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "distributed-correlation_amd",
                        "csrc", "dcor_tables.h")


def read_table(name, cols):
    """A `double name[rows][cols]` table of dcor_tables.h."""
    text = open(TABLES_H).read()
    body = text[text.index(name + "["):]
    body = body[body.index("{") + 1:body.index("};")]
    num = r"\s*(-?0x[0-9a-fp.+-]+)\s*"
    rows = re.findall(r"\{" + ",".join([num] * cols) + r"\}", body)
    return np.array([[float.fromhex(v) for v in row] for row in rows])


def zig_tab():
    """dcor_zig_tab: entry j = 2 L + s is {(-1)^s X[L], X[L+1]}."""
    tab = read_table("dcor_zig_tab", 2)
    assert tab.shape == (2048, 2)
    return tab


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays holding 32-bit words."""
    M0, M1, MASK = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & MASK, (k1 + np.uint64(0xBB67AE85)) & MASK
    return c0, c1, c2, c3


def attempt0(seed, rep, n, tab):
    """Attempt 0 of both normals of samples 0 .. n - 1 of a replicate: for which = 0, 1 the tuple
    (A, H, x0, miss) -- the draw's word and 16-bit field, its fast-path value x0 = fma(d, SX, -SX)
    and whether it misses the fast path (|x0| >= X[L+1])."""
    i = np.arange(n, dtype=np.uint64)
    w0, w1, w2, _ = philox4x32_10(i, rep, SITE_DGP_A, 0, seed & 0xFFFFFFFF, seed >> 32)
    out = []
    for A, H in ((w0, w2 & np.uint64(0xffff)), (w1, w2 >> np.uint64(16))):
        j = (H >> np.uint64(5)).astype(np.int64)
        bits = ((np.uint64(0x3ff00000) | (A >> np.uint64(12))) << np.uint64(32)) | ((A & np.uint64(0xfff)) << np.uint64(20)) \
            | ((H & np.uint64(0x1f)) << np.uint64(15)) | np.uint64(1 << 14)
        d = bits.view(np.float64)
        # fma(d, SX, -SX) = round((d - 1) SX): d - 1 is exact, so the product rounds once
        x0 = (d - 1.0) * tab[j, 0]
        out.append((A, H, x0, ~(np.abs(x0) < tab[j, 1])))
    return out


def slow_samples(seed, rep, n, tab):
    """How many of a replicate's n samples have a normal off the ziggurat's fast path."""
    (_, _, _, m1), (_, _, _, m2) = attempt0(seed, rep, n, tab)
    return int(np.count_nonzero(m1 | m2))
