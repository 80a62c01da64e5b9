"""Shared helpers for the parity tests: seeded synthetic ciphertexts/keys
(splitmix64(seed + limb*2^32 + idx) mod q_limb)."""
import numpy as np

from oracle import binding as ob


def synth_ct(primes, limb_ids, parts, n, seed):
    """[parts][len(limb_ids)][n] uint64, limb j reduced mod primes[limb_ids[j]]."""
    out = np.zeros((parts, len(limb_ids), n), dtype=np.uint64)
    for p in range(parts):
        for j, lid in enumerate(limb_ids):
            out[p, j] = ob.fill_poly(seed * 1000 + p, lid, n, primes[lid])
    return out.reshape(-1)


def synth_key(primes, Q, Qp, n, seed):
    """evaluation key [Q digits][2][Q' limbs][n] (keygeneration.cu:145-185 layout)."""
    out = np.zeros((Q, 2, Qp, n), dtype=np.uint64)
    for i in range(Q):
        for c in range(2):
            for j in range(Qp):
                out[i, c, j] = ob.fill_poly(seed * 100000 + i * 2 + c, j, n, primes[j])
    return out.reshape(-1)


SENTINEL = 0x5555555555555555
# operand layouts (lead, pad) of laid_out: today's packed layout as the control, every item 8 bytes off a 16-byte
# boundary, items that alternate between the two inside one launch, and that alternation starting misaligned
LAYOUTS = {"packed": (0, 0), "off8": (1, 1000), "odd": (0, 1), "off8_odd": (1, 1001)}


def laid_out(items, lead, pad, guard=2):
    """One device buffer: `guard` sentinel words, `lead` (0 or 1) more, the items (equally long uint64 arrays)
    len(item) + pad words apart with sentinels in the gaps, `guard` sentinel words behind the last item.
    Returns (view from the first item on, item stride in words, intact): view.data_ptr() % 16 == 8 * lead, and intact()
    is true while every sentinel word -- the one right in front of the first item included -- still holds."""
    import torch
    import heongpu_amd as hg
    assert lead in (0, 1) and guard >= 2 and guard % 2 == 0 and pad >= 0
    items = [np.ascontiguousarray(x, dtype=np.uint64).reshape(-1) for x in items]
    words = len(items[0])
    assert all(len(x) == words for x in items)
    stride, front = words + pad, guard + lead
    host = np.full(front + (len(items) - 1) * stride + words + guard, SENTINEL, dtype=np.uint64)
    mask = np.ones(len(host), dtype=bool)
    for i, x in enumerate(items):
        host[front + i * stride:front + i * stride + words] = x
        mask[front + i * stride:front + i * stride + words] = False
    buf = hg.to_device(host)
    assert buf.data_ptr() % 16 == 0
    where = torch.from_numpy(np.flatnonzero(mask)).to(buf.device)
    view = buf[front:len(host) - guard]
    assert view.data_ptr() % 16 == 8 * lead

    def intact():
        return bool((buf[where] == SENTINEL).all())

    return view, stride, intact


def items_of(view, stride, words, count):
    """the `count` items of a laid_out view back on the host: [count][words] uint64"""
    import heongpu_amd as hg
    got = hg.to_host(view)
    return np.stack([got[i * stride:i * stride + words] for i in range(count)])


import contextlib  # noqa: E402


@contextlib.contextmanager
def backend_switches(**kw):
    """Options for every context CREATED inside the block (hegpu_context_set_option through
    heongpu_amd.default_options).  The keys are the option names in capitals with the HEGPU_ prefix of the environment
    variables that seed the same defaults (HEGPU_COL_MULTI=1 -> option "col_multi" = 1); the environment itself is
    not touched."""
    import heongpu_amd as hg
    opts = {}
    for k, v in kw.items():
        assert k.startswith("HEGPU_"), k
        opts[k[len("HEGPU_"):].lower()] = int(v)
    with hg.default_options(**opts):
        yield


def extreme_limbs(c, primes, limb_ids, n, pattern, seed):
    """[len(limb_ids)][n] residues at their extremes: 'max' every residue q - 1, 'alt' 0 / q - 1, 'alt3', 'spike' one
    q - 1, 'half' q/2 and q/2 + 1, else seeded random.  Patterns ending in '_coeff' are built in the COEFFICIENT domain
    and transformed on the device, so that the digits a key switch decomposes (after its inverse transform) are the
    extremes."""
    import torch
    import heongpu_amd as hg
    rows = []
    for j, lid in enumerate(limb_ids):
        q = primes[lid]
        base = pattern.replace("_coeff", "")
        if base == "max":
            v = np.full(n, q - 1, dtype=np.uint64)
        elif base == "alt":
            v = np.zeros(n, dtype=np.uint64)
            v[::2] = q - 1
        elif base == "alt3":
            v = np.full(n, q - 1, dtype=np.uint64)
            v[::3] = 0
        elif base == "spike":
            v = np.zeros(n, dtype=np.uint64)
            v[(seed * 7919 + 13 * j) % n] = q - 1
        elif base == "half":
            v = np.full(n, q // 2, dtype=np.uint64)
            v[1::2] = q // 2 + 1
        else:
            v = ob.fill_poly(seed * 1000 + 17, lid, n, q)
        rows.append(v)
    x = np.concatenate(rows)
    if pattern.endswith("_coeff"):
        d = hg.to_device(x)
        assert list(limb_ids) == list(range(len(limb_ids)))
        c.ntt(d, d, False, len(limb_ids), len(limb_ids))
        torch.cuda.synchronize()
        x = hg.to_host(d)
    return x
