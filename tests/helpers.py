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


POISON = 0x0BADC0DE0BADC0DE  # what outputs and workspaces hold before a call of side_stream_and_graph_parity
_busy = []


def _bits(x):
    """a numpy array as the integers of its element size: what the device buffers hold"""
    x = np.ascontiguousarray(x)
    assert x.dtype.itemsize in (4, 8), x.dtype
    return x.reshape(-1).view(np.int64 if x.dtype.itemsize == 8 else np.int32)


def side_stream_and_graph_parity(torch, operands, call, cases, pad=1):
    """The promise of include/hegpu.h -- an entry issues all its work on the caller's stream, allocates nothing and does
    not synchronise -- tested on a stream that is not the null stream, eagerly and from a captured graph.

    operands: name -> (items, kind) as in test_gpu_operand_layout.py: equally long numpy arrays of 8-byte elements (or of
    int32: the TFHE samples), one per item of the batch, and "in", "out", "inout" or "ws".  The arrays give the sizes and
    the warm-up's inputs (zeros are valid input to every entry).  call(d, s) issues the entries on torch's current stream,
    given the device buffers (int64 or int32 tensors) and the item strides by name.  cases: two or more (inputs, want):
    name -> items written over the "in" / "inout" operands, name -> per item the expected leading elements of the "out" /
    "inout" operands, compared bit for bit.

    Every 8-byte operand lies in a buffer of its own between sentinel words, its items `pad` words further apart than
    they are long (laid_out); int32 operands are packed.
      1. warm-up on a side stream: lazy module loading and the function-attribute statics run outside the capture;
      2. the first case eagerly on the side stream while the null stream is busy with long fills queued just before;
         outputs and workspaces hold POISON and the results are read back on the side stream, so a launch or a memset
         that went to the null stream runs late and shows;
      3. POISON again, then the call captured on the side stream alone (torch.cuda.CUDAGraph; no fork or join);
      4. every case: inputs written over the captured buffers, POISON over outputs and workspaces, replay, synchronise,
         compare.  The cases differ from each other and from the warm-up, so nothing left over from an earlier run passes.
    An entry that leaves its stream, allocates or synchronises ends the capture in an error; work that fell outside the
    graph shows as a wrong result at replay.  The sentinels around every operand must hold throughout.
    Returns (d, s) for checks of the caller's own."""
    assert len(cases) >= 2
    dev, d, s, words = {}, {}, {}, {}
    for name, (items, kind) in operands.items():
        assert kind in ("in", "out", "inout", "ws"), kind
        rows = [_bits(x) for x in items]
        words[name] = len(rows[0])
        if rows[0].dtype == np.int64:
            d[name], s[name], intact = laid_out([r.view(np.uint64) for r in rows], 0, pad)
        else:
            d[name], s[name], intact = torch.from_numpy(np.concatenate(rows)).cuda(), words[name], lambda: True
        dev[name] = intact

    def put(name, rows):
        for i, x in enumerate(rows):
            d[name][i * s[name]:i * s[name] + x.numel()].copy_(x)

    def load(inputs):
        for name, (items, kind) in operands.items():
            if kind in ("out", "ws"):
                fill = POISON if d[name].dtype == torch.int64 else POISON & 0x7FFFFFFF
                put(name, [torch.full((words[name],), fill, dtype=d[name].dtype, device="cuda")] * len(items))
            elif name in inputs:
                assert len(inputs[name]) == len(items)
                put(name, [torch.from_numpy(_bits(x)).cuda() for x in inputs[name]])
        torch.cuda.synchronize()

    def compare(want, tag, stream=None):
        # the results are fetched on `stream` alone where one is given: work that went to another stream is not waited for
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            if stream is None:
                torch.cuda.synchronize()
            fetched = {name: d[name].detach().cpu().numpy() for name in want}
        torch.cuda.synchronize()
        for name, intact in dev.items():
            assert intact(), (tag, "written outside the operand " + name)
        for name, rows in want.items():
            got = fetched[name]
            for b, w in enumerate(rows):
                w = _bits(w)
                assert np.array_equal(got[b * s[name]:b * s[name] + len(w)], w), (tag, name, b)

    if not _busy:
        _busy.append(torch.empty(1 << 26, dtype=torch.int64, device="cuda"))  # 512 MiB: one fill takes about 0.2 ms
    side = torch.cuda.Stream()
    load({})
    with torch.cuda.stream(side):
        call(d, s)
    torch.cuda.synchronize()
    inputs, want = cases[0]
    load(inputs)
    for i in range(8):  # the null stream is busy for a millisecond or more; the side stream does not wait for it
        _busy[0].fill_(i)
    with torch.cuda.stream(side):
        call(d, s)
    compare(want, "eager on a side stream", side)
    load({})
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call(d, s)
    for i, (inputs, want) in enumerate(cases):
        load(inputs)
        graph.replay()
        compare(want, "replay %d" % i)
    return d, s


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
