"""Thin Python handle over the C ABI (include/hegpu.h) for tests and bench.

PyTorch is used only for device memory and streams; all arithmetic happens in
libhegpu.so.  Polynomial data is held in torch.int64 tensors that carry the
uint64 bit patterns (torch has no full uint64 support); `to_device`/`to_host`
convert from/to numpy uint64.
"""
import collections
import contextlib
import ctypes

import numpy as np

from . import _lib

BFV, CKKS = 1, 2
SEC_NONE, SEC_128, SEC_192, SEC_256 = 0, 128, 192, 256
TABLES_QP, TABLES_Q_BSK = 0, 1
OP_CKKS_RELIN, OP_CKKS_RESCALE, OP_CKKS_GALOIS, OP_BFV_MULTIPLY, OP_BFV_RELIN, OP_BFV_GALOIS = 1, 2, 3, 4, 5, 6
OP_CKKS_ROTATE_HOISTED = 17
OP_KEYGEN_SECRET, OP_KEYGEN_PUBLIC, OP_KEYGEN_SWITCH, OP_CKKS_ENCRYPT, OP_BFV_ENCRYPT, OP_BFV_DECRYPT, OP_BFV_DECODE = 7, 8, 9, 10, 11, 12, 13
OP_CKKS_ENCODE, OP_CKKS_DECODE = 14, 15
OP_BFV_MULTIPLY_PLAIN = 16
OP_MPC_KEY_SHARE, OP_MPC_BFV_DECRYPT_MERGE = 18, 19
OP_MPC_REFRESH_SHARE, OP_MPC_REFRESH_MERGE = 20, 21
MPC_PUBLIC_KEY, MPC_GALOIS_KEY, MPC_RELIN_ROUND1 = 0, 1, 2
TABLES_PLAIN = 2
OP_CKKS_LOGIC_GATE, OP_BFV_LOGIC_GATE = 22, 23
OP_CKKS_MOD_RAISE = 25  # 24 stays unassigned
OP_CKKS_BOOTSTRAP = 26  # the head of the refresh's workspace; the whole: Context.bootstrap_workspace_bytes
# the gates of the BFV / CKKS logic layer (the TFHE gates keep their own numbering: GATE_*)
LOGIC_AND, LOGIC_OR, LOGIC_XOR, LOGIC_NAND, LOGIC_NOR, LOGIC_XNOR, LOGIC_NOT = range(7)
GATE_B_NONE, GATE_B_CIPHER, GATE_B_PLAIN = 0, 1, 2

E_INVALID, E_LOGIC, E_RUNTIME, E_NODEVICE = 10001, 10002, 10003, 10004


class HEError(RuntimeError):
    """Error returned by the C ABI.  `code` distinguishes the reference's
    exception classes: E_INVALID = std::invalid_argument, E_LOGIC =
    std::logic_error, E_RUNTIME = std::runtime_error; other = hipError_t."""

    def __init__(self, code, msg):
        super().__init__(f"[{code}] {msg}")
        self.code = code


def _check(rc):
    if rc != 0:
        raise HEError(rc, _lib.load().hegpu_last_error().decode())


def _ptr(t):
    if t is None:
        return None
    if isinstance(t, int):
        return t
    return t.data_ptr()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _ws_bytes(ws):
    """the size in bytes of a workspace tensor"""
    return ws.numel() * ws.element_size()


class _Handle:
    """A handle of the C ABI (self._lib, self._h) and the one path of its stream-ordered calls."""

    def _call(self, name, *args, stream=None):
        """hegpu_<name>(handle, *args, stream), the code checked; stream None: torch's current stream"""
        _check(getattr(self._lib, "hegpu_" + name)(self._h, *args, stream if stream is not None else _stream()))


def to_device(arr, device="cuda"):
    import torch
    a = np.ascontiguousarray(arr, dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64)).to(device)


def to_host(t):
    return t.detach().cpu().numpy().view(np.uint64)


_default_options = {}


@contextlib.contextmanager
def default_options(**options):
    """Options (hegpu_context_set_option) applied to every Context CREATED inside the block -- a convenience of
    this ctypes layer for tests and measurements; nothing is written to the environment."""
    old = dict(_default_options)
    _default_options.update(options)
    try:
        yield
    finally:
        _default_options.clear()
        _default_options.update(old)


BCAST_FLAT, BCAST_TREE, BCAST_STAGED, BCAST_SAME_DEVICE = 1, 2, 0x100, 0x200


def broadcast_path_name(path):
    """words for the value of hegpu_last_broadcast_path / *path_out (include/hegpu.h)"""
    if not path:
        return "none (one buffer)"
    shape = {BCAST_FLAT: "flat fan-out from device 0 (every peer directly reachable: one hop)",
             BCAST_TREE: "binomial tree in 32 MiB chunks (some peer not directly reachable from device 0)"}[path & 0xff]
    if path & BCAST_STAGED:
        shape += ", at least one edge WITHOUT peer access (staged through host memory by the runtime)"
    if path & BCAST_SAME_DEVICE:
        shape += ", all buffers on ONE device (functional run)"
    return shape


def broadcast_key(contexts, keys, elems, streams=None):
    """hegpu_broadcast_key: keys[0] (a tensor on contexts[0]'s device) -> keys[i] on contexts[i]'s device.
    Returns the path taken (BCAST_* flags)."""
    n = len(contexts)
    lib = _lib.load()
    hs = (ctypes.c_void_p * n)(*[c._h for c in contexts])
    ks = (ctypes.c_void_p * n)(*[_ptr(k) for k in keys])
    ss = (ctypes.c_void_p * n)(*[s for s in streams]) if streams is not None else None
    _check(lib.hegpu_broadcast_key(hs, n, ks, int(elems), ss))
    return int(lib.hegpu_last_broadcast_path())


def broadcast_bytes(devices, bufs, nbytes, streams=None):
    """hegpu_broadcast_bytes: bufs[0] on devices[0] -> bufs[i] on devices[i] (tensors or addresses).  Returns the path."""
    n = len(devices)
    lib = _lib.load()
    ds = (ctypes.c_int * n)(*[int(d) for d in devices])
    bs = (ctypes.c_void_p * n)(*[_ptr(b) for b in bufs])
    ss = (ctypes.c_void_p * n)(*[s for s in streams]) if streams is not None else None
    path = ctypes.c_int(0)
    _check(lib.hegpu_broadcast_bytes(ds, n, bs, int(nbytes), ss, ctypes.byref(path)))
    return int(path.value)


class Context(_Handle):
    """HEContext<BFV|CKKS>: parameter set + device tables."""

    def __init__(self, handle):
        self._lib = _lib.load()
        self._h = handle
        for k, v in _default_options.items():
            self.set_option(k, v)

    def set_option(self, name, value):
        _check(self._lib.hegpu_context_set_option(self._h, name.encode(), int(value)))

    def clone(self):
        """hegpu_context_clone: the same parameter set and options, not uploaded (one context per device)."""
        h = ctypes.c_void_p()
        _check(self._lib.hegpu_context_clone(self._h, ctypes.byref(h)))
        saved = dict(_default_options)
        _default_options.clear()  # the clone carries the source's options
        try:
            return Context(h)
        finally:
            _default_options.update(saved)

    def upload_device(self, device):
        _check(self._lib.hegpu_context_upload_device(self._h, int(device)))

    @property
    def device(self):
        return self._lib.hegpu_context_device(self._h)

    def get_option(self, name):
        v = ctypes.c_int()
        _check(self._lib.hegpu_context_get_option(self._h, name.encode(), ctypes.byref(v)))
        return v.value

    # -- constructors (mirror set_coeff_modulus_* of the reference) --
    @classmethod
    def from_bit_sizes(cls, scheme, n, log_q, log_p, plain_modulus=0, sec=SEC_128):
        lib = _lib.load()
        q = (ctypes.c_int * len(log_q))(*log_q)
        p = (ctypes.c_int * max(len(log_p), 1))(*log_p)
        h = ctypes.c_void_p()
        _check(lib.hegpu_context_create(scheme, n, q, len(log_q), p, len(log_p), plain_modulus, sec,
                                        ctypes.byref(h)))
        return cls(h)

    @classmethod
    def from_default(cls, scheme, n, p_count=1, plain_modulus=0, sec=SEC_128):
        lib = _lib.load()
        h = ctypes.c_void_p()
        _check(lib.hegpu_context_create_default(scheme, n, p_count, plain_modulus, sec, ctypes.byref(h)))
        return cls(h)

    @classmethod
    def from_primes(cls, scheme, n, primes, q_count, p_count, plain_modulus=0):
        lib = _lib.load()
        arr = (ctypes.c_uint64 * len(primes))(*[int(x) for x in primes])
        h = ctypes.c_void_p()
        _check(lib.hegpu_context_create_from_primes(scheme, n, arr, q_count, p_count, plain_modulus,
                                                    ctypes.byref(h)))
        return cls(h)

    def close(self):
        if self._h:
            self._lib.hegpu_context_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- properties --
    def int(self, name):
        return int(self._lib.hegpu_context_int(self._h, name.encode()))

    @property
    def n_power(self):
        return self.int("n_power")

    @property
    def n(self):
        return 1 << self.n_power

    @property
    def Q_size(self):
        return self.int("Q_size")

    @property
    def P_size(self):
        return self.int("P_size")

    @property
    def Q_prime_size(self):
        return self.int("Q_prime_size")

    @property
    def bsk_modulus(self):
        return self.int("bsk_modulus")

    def table(self, name):
        cnt = self._lib.hegpu_context_get(self._h, name.encode(), None, 0)
        if cnt < 0:
            raise KeyError(name)
        out = np.zeros(cnt, dtype=np.uint64)
        got = self._lib.hegpu_context_get(self._h, name.encode(), out.ctypes.data, cnt)
        assert got == cnt
        return out

    def upload(self):
        _check(self._lib.hegpu_context_upload(self._h))

    def device_ptr(self, name):
        return self._lib.hegpu_context_device_ptr(self._h, name.encode())

    def workspace_bytes(self, op, depth, batch):
        return int(self._lib.hegpu_workspace_bytes(self._h, op, depth, batch))

    def workspace(self, op, depth, batch, device="cuda"):
        import torch
        nbytes = self.workspace_bytes(op, depth, batch)
        return torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=device)

    # -- NTT seam --
    def ntt(self, src, dst, inverse, batch, mod_count, mod_offset=0, mod_order=None, poly_order=None,
            table_set=TABLES_QP, stream=None):
        self._call("ntt", table_set, _ptr(src), _ptr(dst), int(inverse), batch, mod_count, mod_offset, _ptr(mod_order),
                   _ptr(poly_order), stream=stream)

    # -- kernels --
    def addition(self, a, b, out, limbs, parts, batch=1, op=0, stream=None):
        self._call("addition", _ptr(a), _ptr(b), _ptr(out), limbs, parts, batch, op, stream=stream)

    def cross_multiplication(self, in1, s1, in2, s2, out, so, decomp_size, batch=1, table_set=TABLES_QP,
                             stream=None):
        self._call("cross_multiplication", table_set, _ptr(in1), s1, _ptr(in2), s2, _ptr(out), so, decomp_size, batch,
                   stream=stream)

    def cipher_broadcast(self, src, s_in, out, s_out, digits, nmods, split, level, batch=1, stream=None):
        self._call("cipher_broadcast", _ptr(src), s_in, _ptr(out), s_out, digits, nmods, split, level, batch,
                   stream=stream)

    def keyswitch_multiply_accumulate(self, src, s_in, key, out, s_out, digits, nmods, key_limbs, split, level,
                                      batch=1, stream=None):
        self._call("keyswitch_multiply_accumulate", _ptr(src), s_in, _ptr(key), _ptr(out), s_out, digits, nmods,
                   key_limbs, split, level, batch, stream=stream)

    def base_conversion_DtoQtilde(self, src, s_in, out, s_out, depth=0, batch=1, stream=None):
        self._call("base_conversion_DtoQtilde", _ptr(src), s_in, _ptr(out), s_out, depth, batch, stream=stream)

    def divide_round_lastq(self, src, s_in, ct, s_ct, out, s_out, switchkey=0, batch=1, stream=None):
        self._call("divide_round_lastq", _ptr(src), s_in, _ptr(ct), s_ct, _ptr(out), s_out, switchkey, batch,
                   stream=stream)

    def divide_round_lastq_permute(self, src, s_in, in2, s_in2, out, s_out, galois_elt, depth=0, batch=1,
                                   stream=None):
        self._call("divide_round_lastq_permute", _ptr(src), s_in, _ptr(in2), s_in2, _ptr(out), s_out, galois_elt, depth,
                   batch, stream=stream)

    def divide_round_lastq_leveled_stage_one(self, src, s_in, out, s_out, rescale=0, depth=0, batch=1, stream=None):
        self._call("divide_round_lastq_leveled_stage_one", _ptr(src), s_in, _ptr(out), s_out, rescale, depth, batch,
                   stream=stream)

    def divide_round_lastq_leveled_stage_two(self, last, s_last, src, s_in, ct, s_ct, out, s_out, switchkey=0, depth=0,
                                             batch=1, stream=None):
        self._call("divide_round_lastq_leveled_stage_two", _ptr(last), s_last, _ptr(src), s_in, _ptr(ct), s_ct,
                   _ptr(out), s_out, switchkey, depth, batch, stream=stream)

    def move_cipher_leveled(self, src, s_in, out, s_out, depth=0, batch=1, stream=None):
        self._call("move_cipher_leveled", _ptr(src), s_in, _ptr(out), s_out, depth, batch, stream=stream)

    def divide_round_lastq_rescale(self, last, s_last, src, s_in, out, s_out, depth=0, batch=1, stream=None):
        self._call("divide_round_lastq_rescale", _ptr(last), s_last, _ptr(src), s_in, _ptr(out), s_out, depth, batch,
                   stream=stream)

    def divide_round_lastq_extended(self, src, s_in, ct, s_ct, out, s_out, mode=0, depth=0, batch=1, stream=None):
        self._call("divide_round_lastq_extended", _ptr(src), s_in, _ptr(ct) if ct is not None else None, s_ct,
                   _ptr(out), s_out, mode, depth, batch, stream=stream)

    def fast_convertion(self, in1, s1, in2, s2, out, so, batch=1, stream=None):
        self._call("fast_convertion", _ptr(in1), s1, _ptr(in2), s2, _ptr(out), so, batch, stream=stream)

    def fast_floor(self, src, si, out, so, batch=1, stream=None):
        self._call("fast_floor", _ptr(src), si, _ptr(out), so, batch, stream=stream)

    # -- operators (HEArithmeticOperator) --
    def ckks_multiply(self, ct1, s1, ct2, s2, out, so, depth=0, batch=1, stream=None):
        self._call("ckks_multiply", _ptr(ct1), s1, _ptr(ct2), s2, _ptr(out), so, depth, batch, stream=stream)

    def ckks_relinearize_inplace(self, ct, cs, key, depth, batch, ws, stream=None):
        self._call("ckks_relinearize_inplace", _ptr(ct), cs, _ptr(key), depth, batch, _ptr(ws), _ws_bytes(ws),
                   stream=stream)

    def probe_ckks_relinearize(self, ct, cs, key, depth, batch, ws, phases, stream=None):
        """measurement seam: only the launches selected by `phases` (include/hegpu.h)"""
        self._call("probe_ckks_relinearize", _ptr(ct), cs, _ptr(key), depth, batch, _ptr(ws), _ws_bytes(ws), phases,
                   stream=stream)

    def ckks_rescale_inplace(self, ct, cs, depth, batch, ws, stream=None):
        self._call("ckks_rescale_inplace", _ptr(ct), cs, depth, batch, _ptr(ws), _ws_bytes(ws), stream=stream)

    def ckks_apply_galois(self, ct, cs, out, so, key, galois_elt, depth, batch, ws, stream=None):
        self._call("ckks_apply_galois", _ptr(ct), cs, _ptr(out), so, _ptr(key), galois_elt, depth, batch, _ptr(ws),
                   _ws_bytes(ws), stream=stream)

    def mod_raise(self, src, s_in, out, s_out, limbs, parts=2, batch=1, stream=None):
        """hegpu_mod_raise: src [parts][1][N] at q_0 (coefficient domain) -> out [parts][limbs][N], the centred lift"""
        self._call("mod_raise", _ptr(src), s_in, _ptr(out), s_out, limbs, parts, batch, stream=stream)

    def ckks_mod_raise(self, ct, cs, out, so, out_depth, batch, ws, ws_bytes=None, stream=None):
        """hegpu_ckks_mod_raise: ct [2][1][N] at depth Q - 1 -> out [2][Q - out_depth][N], both in the NTT domain.
        Workspace OP_CKKS_MOD_RAISE (ws_bytes: its size when ws is an address, not a tensor)"""
        self._call("ckks_mod_raise", _ptr(ct), cs, _ptr(out), so, out_depth, batch, _ptr(ws),
                   _ws_bytes(ws) if ws_bytes is None else ws_bytes, stream=stream)

    def ckks_rotate_hoisted(self, ct, cs, out, so, keys, galois_elts, depth, batch, ws, stream=None):
        """fast_single_hoisting_rotation_ckks: keys = list of device tensors (None where galois_elts[i] == 0)"""
        cnt = len(galois_elts)
        kp = (ctypes.c_void_p * cnt)(*[(_ptr(k) if k is not None else None) for k in keys])
        ge = (ctypes.c_int * cnt)(*[int(g) for g in galois_elts])
        self._call("ckks_rotate_hoisted", _ptr(ct), cs, _ptr(out), so, kp, ge, cnt, depth, batch, _ptr(ws),
                   _ws_bytes(ws), stream=stream)

    def ckks_diag_mac(self, rot, rot_stride, n1, diags, n_diag, index, n2, out, out_stride, depth=0, batch=1, stream=None):
        """hegpu_ckks_diag_mac: index = n2 rows of n1 packed-diagonal numbers (-1: absent)"""
        ix = (ctypes.c_int * (n1 * n2))(*[int(v) for row in index for v in row])
        self._call("ckks_diag_mac", _ptr(rot), rot_stride, n1, _ptr(diags), n_diag, ix, n2, _ptr(out), out_stride,
                   depth, batch, stream=stream)

    def linear_transform_workspace_bytes(self, n1, n2, depth, batch):
        return int(self._lib.hegpu_ckks_linear_transform_workspace_bytes(self._h, n1, n2, depth, batch))

    def ckks_linear_transform(self, ct, cs, out, so, diags, n_diag, index, baby_keys, baby_elts, giant_keys, giant_elts,
                              depth, batch, ws, stream=None, giant_parent=None):
        """hegpu_ckks_linear_transform: keys = lists of device tensors (None where the element is 0).  giant_parent (a list
        of n2 term numbers, -1 = a root; giant_step_chain): hegpu_ckks_linear_transform_chained, giant_keys / giant_elts
        are then the links of the chain"""
        n1, n2 = len(baby_elts), len(giant_elts)
        ix = (ctypes.c_int * (n1 * n2))(*[int(v) for row in index for v in row])
        bk = (ctypes.c_void_p * n1)(*[(_ptr(k) if k is not None else None) for k in baby_keys])
        gk = (ctypes.c_void_p * n2)(*[(_ptr(k) if k is not None else None) for k in giant_keys])
        be = (ctypes.c_int * n1)(*[int(g) for g in baby_elts])
        ge = (ctypes.c_int * n2)(*[int(g) for g in giant_elts])
        if giant_parent is None:
            self._call("ckks_linear_transform", _ptr(ct), cs, _ptr(out), so, _ptr(diags), n_diag, ix, n1, n2, bk, be, gk,
                       ge, depth, batch, _ptr(ws), _ws_bytes(ws), stream=stream)
            return
        if len(giant_parent) != n2:
            raise ValueError("giant_parent has one entry per giant step")
        gp = (ctypes.c_int * max(n2, 1))(*[int(p) for p in giant_parent])
        self._call("ckks_linear_transform_chained", _ptr(ct), cs, _ptr(out), so, _ptr(diags), n_diag, ix, n1, n2, bk, be,
                   gk, ge, gp, depth, batch, _ptr(ws), _ws_bytes(ws), stream=stream)

    def ckks_conj_split(self, x, xs, xc, xcs, out0, out1, so, depth, out_depth, batch=1, stream=None):
        """hegpu_ckks_conj_split: out0 = x + xc, out1 = div_i(x - xc) on the Q - out_depth kept limbs"""
        self._call("ckks_conj_split", _ptr(x), xs, _ptr(xc), xcs, _ptr(out0), _ptr(out1), so, depth, out_depth, batch,
                   stream=stream)

    def ckks_conj_merge(self, c0, s0, c1, s1, out, so, depth, out_depth, batch=1, stream=None):
        """hegpu_ckks_conj_merge: out = c0 + mult_i(c1) on the Q - out_depth kept limbs"""
        self._call("ckks_conj_merge", _ptr(c0), s0, _ptr(c1), s1, _ptr(out), so, depth, out_depth, batch, stream=stream)

    def ckks_weighted_sum(self, terms, strides, term_limbs, weights, w0, out, so, limbs, batch=1, stream=None):
        """hegpu_ckks_weighted_sum: out = w0 + sum_k weights[k] * terms[k] on the first `limbs` limbs.  terms: device tensors
        [2][term_limbs[k]][N] per item; weights / w0: complex numbers whose parts are rounded to integers"""
        k = len(terms)
        tp = (ctypes.c_void_p * max(k, 1))(*[_ptr(t) for t in terms])
        ts = (ctypes.c_uint64 * max(k, 1))(*[int(v) for v in strides])
        tl = (ctypes.c_int * max(k, 1))(*[int(v) for v in term_limbs])
        tw = (ctypes.c_double * max(2 * k, 1))(*[v for w in weights for v in (complex(w).real, complex(w).imag)])
        self._call("ckks_weighted_sum", tp, ts, tl, tw, k, complex(w0).real, complex(w0).imag, _ptr(out), so, limbs,
                   batch, stream=stream)

    def ckks_double_sub(self, a, a_stride, a_limbs, b, b_stride, b_limbs, value, out, so, limbs, batch=1, stream=None):
        """hegpu_ckks_double_sub: out = 2 a - b on the first `limbs` limbs; b None: round(value) leaves part 0 instead"""
        self._call("ckks_double_sub", _ptr(a), a_stride, a_limbs, _ptr(b), b_stride, b_limbs, float(value), _ptr(out),
                   so, limbs, batch, stream=stream)

    def ckks_gate_combine(self, gate, a, a_stride, a_limbs, b, b_kind, b_stride, b_limbs, p, p_stride, p_limbs, scale_one,
                          out, so, limbs, batch=1, stream=None):
        """hegpu_ckks_gate_combine: out = c0 * one + c1 * (a + b) + c2 * p on the first `limbs` limbs, one pass"""
        self._call("ckks_gate_combine", gate, _ptr(a), a_stride, a_limbs, _ptr(b), b_kind, b_stride, b_limbs, _ptr(p),
                   p_stride, p_limbs, float(scale_one), _ptr(out), so, limbs, batch, stream=stream)

    def bfv_gate_combine(self, gate, a, a_stride, b, b_kind, b_stride, p, p_stride, out, so, batch=1, stream=None):
        """hegpu_bfv_gate_combine: the same in the coefficient domain, every operand at Q limbs"""
        self._call("bfv_gate_combine", gate, _ptr(a), a_stride, _ptr(b), b_kind, b_stride, _ptr(p), p_stride, _ptr(out),
                   so, batch, stream=stream)

    def ckks_logic_gate(self, gate, a, a_stride, b, b_kind, b_stride, relin_key, scale_one, out, so, depth, batch, ws,
                        stream=None):
        """hegpu_ckks_logic_gate: product sequence + one combine pass; out at depth + 1 (NOT: depth)"""
        self._call("ckks_logic_gate", gate, _ptr(a), a_stride, _ptr(b), b_kind, b_stride, _ptr(relin_key),
                   float(scale_one), _ptr(out), so, depth, batch, _ptr(ws), _ws_bytes(ws) if ws is not None else 0,
                   stream=stream)

    def bfv_logic_gate(self, gate, a, a_stride, b, b_kind, b_stride, relin_key, out, so, batch, ws, stream=None):
        """hegpu_bfv_logic_gate: product sequence + one combine pass, coefficient domain"""
        self._call("bfv_logic_gate", gate, _ptr(a), a_stride, _ptr(b), b_kind, b_stride, _ptr(relin_key), _ptr(out), so,
                   batch, _ptr(ws), _ws_bytes(ws) if ws is not None else 0, stream=stream)

    def poly_eval_workspace_bytes(self, plan, depth, batch):
        return int(self._lib.hegpu_ckks_poly_eval_workspace_bytes(self._h, plan.steps, len(plan.steps), depth, batch))

    def ckks_poly_eval(self, ct, cs, out, so, plan, relin_key, depth, batch, ws, stream=None):
        """hegpu_ckks_poly_eval: executes a PolyEvalPlan (poly_eval_plan) made for the level Q - 1 - depth; the result is
        at depth Q - 1 - plan.level and scale plan.scale"""
        self._call("ckks_poly_eval", _ptr(ct), cs, _ptr(out), so, plan.steps, len(plan.steps), _ptr(relin_key), depth,
                   batch, _ptr(ws), _ws_bytes(ws), stream=stream)

    @staticmethod
    def linear_factors(factors, chained=False, galois_key=None, n=None):
        """the hegpu_linear_factor array of a sequence entry.  factors: one (diags, n_diag, index, baby_keys, baby_elts,
        giant_keys, giant_elts) per matrix, the arguments of ckks_linear_transform, or the same with giant_parent as an
        eighth entry (None = direct), giant_keys / giant_elts then being the links.  Returns (array, keep-alive).
        chained=True: every factor is (diags, n_diag, index, baby_keys, baby_elts, giant_shifts) with the plan's giant
        shifts; its links come from giant_step_chain over N = n, their keys from galois_key(elt) -> device key.  Returns
        (array, keep-alive, link_shifts): the distinct non-zero link shifts, all the giant-step keys the factors need."""
        needed = set()
        if chained:
            made = []
            for diags, n_diag, index, baby_keys, baby_elts, giant_shifts in factors:
                keys, elts, parent, links = chained_giant_steps(giant_shifts, n, galois_key)
                needed.update(s for s in links if s)
                made.append((diags, n_diag, index, baby_keys, baby_elts, keys, elts, parent))
            factors = made
        arr = (_lib.LinearFactor * len(factors))()
        keep = []
        for f, factor in zip(arr, factors):
            diags, n_diag, index, baby_keys, baby_elts, giant_keys, giant_elts = factor[:7]
            n1, n2 = len(baby_elts), len(giant_elts)
            ix = (ctypes.c_int * (n1 * n2))(*[int(v) for row in index for v in row])
            bk = (ctypes.c_void_p * n1)(*[(_ptr(k) if k is not None else None) for k in baby_keys])
            gk = (ctypes.c_void_p * n2)(*[(_ptr(k) if k is not None else None) for k in giant_keys])
            be = (ctypes.c_int * n1)(*[int(g) for g in baby_elts])
            ge = (ctypes.c_int * n2)(*[int(g) for g in giant_elts])
            f.diags, f.n_diag, f.index, f.n1, f.n2 = _ptr(diags), n_diag, ix, n1, n2
            f.baby_keys, f.baby_elts, f.giant_keys, f.giant_elts = bk, be, gk, ge
            keep += [ix, bk, gk, be, ge, diags, baby_keys, giant_keys]
            if len(factor) > 7 and factor[7] is not None:
                if len(factor[7]) != n2:
                    raise ValueError("giant_parent has one entry per giant step")
                gp = (ctypes.c_int * n2)(*[int(p) for p in factor[7]])
                f.giant_parent = gp
                keep.append(gp)
        return (arr, keep, sorted(needed)) if chained else (arr, keep)

    def encoding_transform_workspace_bytes(self, factors, depth, batch):
        arr, _keep = self.linear_factors(factors)
        return int(self._lib.hegpu_ckks_encoding_transform_workspace_bytes(self._h, arr, len(factors), depth, batch))

    def ckks_coeff_to_slot(self, ct, cs, out0, out1, so, factors, conj_key, depth, batch, ws, stream=None):
        """hegpu_ckks_coeff_to_slot: factors as for linear_factors, their diagonals encoded at depth + position"""
        arr, _keep = self.linear_factors(factors)
        self._call("ckks_coeff_to_slot", _ptr(ct), cs, _ptr(out0), _ptr(out1), so, arr, len(factors), _ptr(conj_key),
                   depth, batch, _ptr(ws), _ws_bytes(ws), stream=stream)

    def ckks_slot_to_coeff(self, c0, s0, c1, s1, out, so, factors, depth, batch, ws, stream=None):
        """hegpu_ckks_slot_to_coeff: factors as for linear_factors, their diagonals encoded at depth + 1 + position"""
        arr, _keep = self.linear_factors(factors)
        self._call("ckks_slot_to_coeff", _ptr(c0), s0, _ptr(c1), s1, _ptr(out), so, arr, len(factors), depth, batch,
                   _ptr(ws), _ws_bytes(ws), stream=stream)

    def bootstrap_workspace_bytes(self, plan, cts, stc, switch_keys, batch):
        """hegpu_ckks_bootstrap_workspace_bytes; plan: a BootstrapPlan (bootstrap_plan), cts / stc as for linear_factors"""
        a, _ka = self.linear_factors(cts)
        b, _kb = self.linear_factors(stc)
        return int(self._lib.hegpu_ckks_bootstrap_workspace_bytes(self._h, ctypes.byref(plan.c), plan.eval_mod.steps,
                                                                  len(plan.eval_mod.steps), a, len(cts), b, len(stc),
                                                                  int(bool(switch_keys)), batch))

    def ckks_bootstrap(self, ct, cs, out, so, plan, cts, stc, conj_key, relin_key, batch, ws, swk_dense_to_sparse=None,
                       swk_sparse_to_dense=None, stream=None):
        """hegpu_ckks_bootstrap: ct [2][1][N] per item at q_0 -> out [2][plan.out_level + 1][N] at plan.out_scale (room for
        one limb more per part on the way).  cts / stc: as for linear_factors (bootstrap_factors builds them)"""
        a, _ka = self.linear_factors(cts)
        b, _kb = self.linear_factors(stc)
        self._call("ckks_bootstrap", _ptr(ct), cs, _ptr(out), so, ctypes.byref(plan.c), plan.eval_mod.steps,
                   len(plan.eval_mod.steps), a, len(cts), b, len(stc), _ptr(conj_key), _ptr(relin_key),
                   _ptr(swk_dense_to_sparse), _ptr(swk_sparse_to_dense), batch, _ptr(ws),
                   _ws_bytes(ws) if ws is not None else 0, stream=stream)

    def bootstrap_factors(self, plan, galois_key, encode=None, chained=False):
        """The two factor lists of Context.ckks_bootstrap from a BootstrapPlan: the factorisation of the special FFT
        (encoding_transform_factors), each factor's baby-step/giant-step plan (linear_transform_plan) and its diagonals
        encoded at the level and scale the plan gives them.  galois_key(elt) -> device key of a Galois element;
        encode(values, scale, limbs) -> packed residues [limbs][N] of one diagonal (default: ckks_encode_ex mode 1).
        Returns (cts, stc, galois_elts): the lists and every element used, the conjugation 2N - 1 included.
        chained=True: every factor's giant steps are chained (giant_step_chain); the factors carry giant_parent and their
        links, and galois_elts is the reduced set: baby steps, links and the conjugation."""
        import torch
        n, slots = self.n, self.n // 2
        if encode is None:
            def encode(values, scale, limbs):
                return self.ckks_encode_ex(1, torch.from_numpy(np.ascontiguousarray(values)).cuda(), scale)[:limbs * n]
        elts = set()

        def key(shift):
            if not shift:
                return None, 0
            e = steps_to_galois_elt(shift, n, 5)
            elts.add(e)
            return galois_key(e), e

        def side(inverse, pieces, first_level, scales):
            out = []
            for f, g in enumerate(encoding_transform_factors(n, inverse, pieces)):
                lp = linear_transform_plan(g.offsets, slots, stride=g.stride)
                limbs = first_level - f + 1
                order = np.argsort([k % slots for k in g.offsets])  # the plan numbers the diagonals by k mod slots
                packed = torch.cat([encode(np.roll(g.diagonals[order[p]], -lp.pre_rotation[p]), scales[f], limbs)
                                    for p in range(len(order))])
                chain = giant_step_chain(lp.giant_shifts, slots) if chained else None
                baby = [key(s) for s in lp.baby_shifts]
                giant = [key(s) for s in (chain.link_shifts if chained else lp.giant_shifts)]
                out.append((packed, len(order), lp.index, [k for k, _ in baby], [e for _, e in baby], [k for k, _ in giant],
                            [e for _, e in giant]) + ((chain.parent,) if chained else ()))
            return out

        # a SlimBootstrapPlan's SlotToCoeff starts at the input's own level: there is no merge below it
        stc_first = plan.in_level if isinstance(plan, SlimBootstrapPlan) else plan.stc_level - 1
        cts = side(True, plan.cts_pieces, plan.cts_level, plan.cts_scale)
        stc = side(False, plan.stc_pieces, stc_first, plan.stc_scale)
        elts.add(2 * n - 1)
        return cts, stc, sorted(elts)

    def slim_bootstrap_factors(self, plan, galois_key, encode=None, chained=False):
        """bootstrap_factors for a SlimBootstrapPlan (slim_bootstrap_plan): the same factorisation and encoder, SlotToCoeff
        factor g at level plan.in_level - g and scale plan.stc_scale[g].  Returns (cts, stc, galois_elts)."""
        return self.bootstrap_factors(plan, galois_key, encode, chained)

    def slim_bootstrap_workspace_bytes(self, plan, cts, stc, batch):
        """hegpu_ckks_slim_bootstrap_workspace_bytes; plan: a SlimBootstrapPlan, cts / stc as for linear_factors"""
        a, _ka = self.linear_factors(cts)
        b, _kb = self.linear_factors(stc)
        return int(self._lib.hegpu_ckks_slim_bootstrap_workspace_bytes(self._h, ctypes.byref(plan.c), plan.trig.steps,
                                                                       len(plan.trig.steps), a, len(cts), b, len(stc), batch))

    def ckks_slim_bootstrap(self, ct, cs, out, so, plan, cts, stc, conj_key, relin_key, batch, ws, ct2=None, cs2=0,
                            stream=None):
        """hegpu_ckks_slim_bootstrap: ct (and ct2 for a gate) [2][plan.in_level + 1][N] per item -> out
        [2][plan.out_level + 1][N] at plan.out_scale (room for plan.trig.out_limbs limbs per part on the way)"""
        a, _ka = self.linear_factors(cts)
        b, _kb = self.linear_factors(stc)
        self._call("ckks_slim_bootstrap", _ptr(ct), cs, _ptr(ct2), cs2, _ptr(out), so, ctypes.byref(plan.c),
                   plan.trig.steps, len(plan.trig.steps), a, len(cts), b, len(stc), _ptr(conj_key), _ptr(relin_key), batch,
                   _ptr(ws), _ws_bytes(ws) if ws is not None else 0, stream=stream)

    def ckks_conj_real(self, x, xs, xc, xcs, out, so, depth, out_depth, batch=1, stream=None):
        """hegpu_ckks_conj_real: out = x + xc on the Q - out_depth kept limbs (conj_split's out0 alone)"""
        self._call("ckks_conj_real", _ptr(x), xs, _ptr(xc), xcs, _ptr(out), so, depth, out_depth, batch, stream=stream)

    def bfv_multiply(self, ct1, s1, ct2, s2, out, so, batch, ws, stream=None):
        self._call("bfv_multiply", _ptr(ct1), s1, _ptr(ct2), s2, _ptr(out), so, batch, _ptr(ws), _ws_bytes(ws),
                   stream=stream)

    def bfv_relinearize_inplace(self, ct, cs, key, batch, ws, stream=None):
        self._call("bfv_relinearize_inplace", _ptr(ct), cs, _ptr(key), batch, _ptr(ws), _ws_bytes(ws), stream=stream)

    def bfv_apply_galois(self, ct, cs, out, so, key, galois_elt, batch, ws, stream=None):
        self._call("bfv_apply_galois", _ptr(ct), cs, _ptr(out), so, _ptr(key), galois_elt, batch, _ptr(ws),
                   _ws_bytes(ws), stream=stream)


    # ---- key generation / encryption / decryption (method I keys)
    def _kg_ws(self, op):
        return self.workspace(op, 0, 1)

    def generate_secret_key(self, rng, hamming_weight=None, stream=None):
        import torch
        n, Qp = self.n, self.Q_prime_size
        sk = torch.empty(Qp * n, dtype=torch.int64, device="cuda")
        ws = self._kg_ws(OP_KEYGEN_SECRET)
        hw = n // 2 if hamming_weight is None else hamming_weight  # secretkey.cu:23
        self._call("generate_secret_key", rng._h, hw, _ptr(sk), _ptr(ws), _ws_bytes(ws), stream=stream)
        return sk

    def generate_public_key(self, rng, sk, stream=None):
        import torch
        pk = torch.empty(2 * self.Q_prime_size * self.n, dtype=torch.int64, device="cuda")
        ws = self._kg_ws(OP_KEYGEN_PUBLIC)
        self._call("generate_public_key", rng._h, _ptr(sk), _ptr(pk), _ptr(ws), _ws_bytes(ws), stream=stream)
        return pk

    def switch_key_digits(self):
        """digits of a key-switching key: Q (method I) or the depth-0 partition of method II
        (digits of 2 primes for BFV, of P_size primes for CKKS; contextpool.cpp:161-438)"""
        if self.P_size == 1:
            return self.Q_size
        m = 2 if self.int("scheme") == BFV else self.P_size
        return -(-self.Q_size // m)

    def generate_relin_key(self, rng, sk, stream=None):
        import torch
        rk = torch.empty(self.switch_key_digits() * 2 * self.Q_prime_size * self.n, dtype=torch.int64, device="cuda")
        ws = self._kg_ws(OP_KEYGEN_SWITCH)
        self._call("generate_relin_key", rng._h, _ptr(sk), _ptr(rk), _ptr(ws), _ws_bytes(ws), stream=stream)
        return rk

    def generate_switch_key(self, rng, new_sk, old_sk, stream=None):
        """HEKeyGenerator::generate_switch_key (ckks/keygenerator.cu:996-1095): key under new_sk carrying old_sk."""
        import torch
        swk = torch.empty(self.switch_key_digits() * 2 * self.Q_prime_size * self.n, dtype=torch.int64, device="cuda")
        ws = self._kg_ws(OP_KEYGEN_SWITCH)
        self._call("generate_switch_key", rng._h, _ptr(new_sk), _ptr(old_sk), _ptr(swk), _ptr(ws), _ws_bytes(ws),
                   stream=stream)
        return swk

    def generate_galois_key(self, rng, sk, galois_elt, stream=None):
        import torch
        gk = torch.empty(self.switch_key_digits() * 2 * self.Q_prime_size * self.n, dtype=torch.int64, device="cuda")
        ws = self._kg_ws(OP_KEYGEN_SWITCH)
        self._call("generate_galois_key", rng._h, _ptr(sk), galois_elt, _ptr(gk), _ptr(ws), _ws_bytes(ws),
                   stream=stream)
        return gk

    def ckks_encrypt(self, rng, pk, plain, stream=None):
        import torch
        ct = torch.empty(2 * self.Q_size * self.n, dtype=torch.int64, device="cuda")
        ws = self._kg_ws(OP_CKKS_ENCRYPT)
        self._call("ckks_encrypt", rng._h, _ptr(pk), _ptr(plain), _ptr(ct), _ptr(ws), _ws_bytes(ws), stream=stream)
        return ct

    def bfv_encrypt(self, rng, pk, plain, stream=None):
        import torch
        ct = torch.empty(2 * self.Q_size * self.n, dtype=torch.int64, device="cuda")
        ws = self._kg_ws(OP_BFV_ENCRYPT)
        self._call("bfv_encrypt", rng._h, _ptr(pk), _ptr(plain), _ptr(ct), _ptr(ws), _ws_bytes(ws), stream=stream)
        return ct

    def bfv_decrypt(self, ct, sk, stream=None):
        import torch
        plain = torch.empty(self.n, dtype=torch.int64, device="cuda")
        ws = self._kg_ws(OP_BFV_DECRYPT)
        self._call("bfv_decrypt", _ptr(ct), _ptr(sk), _ptr(plain), _ptr(ws), _ws_bytes(ws), stream=stream)
        return plain

    def bfv_encode(self, message, stream=None):
        """message: device int64 tensor with at most N entries"""
        import torch
        plain = torch.empty(self.n, dtype=torch.int64, device="cuda")
        self._call("bfv_encode", _ptr(message), message.numel(), _ptr(plain), stream=stream)
        return plain

    def bfv_decode(self, plain, stream=None):
        import torch
        out = torch.empty(self.n, dtype=torch.int64, device="cuda")
        ws = self._kg_ws(OP_BFV_DECODE)
        self._call("bfv_decode", _ptr(plain), _ptr(out), _ptr(ws), _ws_bytes(ws), stream=stream)
        return out

    def ckks_encode(self, message, scale, stream=None):
        """message: device float64 tensor with at most N/2 entries"""
        import torch
        plain = torch.empty(self.Q_size * self.n, dtype=torch.int64, device="cuda")
        ws = self._kg_ws(OP_CKKS_ENCODE)
        self._call("ckks_encode", _ptr(message), message.numel(), float(scale), _ptr(plain), _ptr(ws), _ws_bytes(ws),
                   stream=stream)
        return plain

    def ckks_decode(self, plain, scale, depth=0, stream=None):
        import torch
        out = torch.empty(self.n // 2, dtype=torch.float64, device="cuda")
        ws = self.workspace(OP_CKKS_DECODE, depth, 1)
        self._call("ckks_decode", _ptr(plain), depth, float(scale), _ptr(out), _ptr(ws), _ws_bytes(ws), stream=stream)
        return out

    def bfv_plain_to_ntt(self, plain, stream=None):
        import torch
        out = torch.empty(self.Q_size * self.n, dtype=torch.int64, device="cuda")
        self._call("bfv_plain_to_ntt", _ptr(plain), _ptr(out), stream=stream)
        return out

    def negacyclic_shift(self, ct, shift, limbs, parts=2, stream=None):
        import torch
        out = torch.empty(parts * limbs * self.n, dtype=torch.int64, device="cuda")
        self._call("negacyclic_shift", _ptr(ct), _ptr(out), shift, limbs, parts, stream=stream)
        return out

    def ckks_constant_op(self, op, ct, value, limbs, parts=2, out=None, stream=None):
        """op 0/1/2 = add / subtract / multiply by round(value) (value = constant * scale); NTT-domain ciphertext"""
        import torch
        if out is None:
            out = torch.empty(parts * limbs * self.n, dtype=torch.int64, device="cuda")
        self._call("ckks_constant_op", op, _ptr(ct), float(value), _ptr(out), limbs, parts, stream=stream)
        return out

    def ckks_gaussian_integer_op(self, op, ct, re, im, limbs, parts=2, out=None, stream=None):
        """op 0 / 1 = add / multiply by the constant round(re) + round(im) i in every slot"""
        import torch
        if out is None:
            out = torch.empty(parts * limbs * self.n, dtype=torch.int64, device="cuda")
        self._call("ckks_gaussian_integer_op", op, _ptr(ct), float(re), float(im), _ptr(out), limbs, parts,
                   stream=stream)
        return out

    def ckks_mult_i(self, ct, limbs, parts=2, divide=False, out=None, stream=None):
        import torch
        if out is None:
            out = torch.empty(parts * limbs * self.n, dtype=torch.int64, device="cuda")
        self._call("ckks_mult_i", _ptr(ct), _ptr(out), limbs, parts, int(divide), stream=stream)
        return out

    def ckks_encode_ex(self, mode, message, scale, stream=None):
        """The other encodings of HEEncoder<CKKS> (ckks/encoder.cu:222-446).  mode 1: complex128 device
        tensor (<= N/2) into the slots; mode 2: float64 device tensor (<= N) as polynomial coefficients;
        mode 3: `message` is one Python number placed in every slot."""
        import torch
        plain = torch.empty(self.Q_size * self.n, dtype=torch.int64, device="cuda")
        if mode == 3:
            self._call("ckks_encode_scalar", float(message), float(scale), _ptr(plain), stream=stream)
        elif mode == 2:
            self._call("ckks_encode_coeff", _ptr(message), message.numel(), float(scale), _ptr(plain), stream=stream)
        else:
            assert mode == 1 and message.dtype == torch.complex128
            ws = self._kg_ws(OP_CKKS_ENCODE)
            self._call("ckks_encode_complex", _ptr(message), message.numel(), float(scale), _ptr(plain), _ptr(ws),
                       _ws_bytes(ws), stream=stream)
        return plain

    def ckks_decode_ex(self, mode, plain, scale, depth=0, stream=None):
        """mode 1: the N/2 complex slots; mode 2: the N polynomial coefficients"""
        import torch
        ws = self.workspace(OP_CKKS_DECODE, depth, 1)
        if mode == 1:
            out = torch.empty(self.n // 2, dtype=torch.complex128, device="cuda")
        else:
            out = torch.empty(self.n, dtype=torch.float64, device="cuda")
        self._call("ckks_decode_complex" if mode == 1 else "ckks_decode_coeff", _ptr(plain), depth, float(scale), _ptr(out),
                   _ptr(ws), _ws_bytes(ws), stream=stream)
        return out

    def ckks_decrypt(self, ct, sk, depth=0, stream=None):
        import torch
        plain = torch.empty((self.Q_size - depth) * self.n, dtype=torch.int64, device="cuda")
        self._call("ckks_decrypt", _ptr(ct), _ptr(sk), depth, _ptr(plain), stream=stream)
        return plain

    # ---- N-out-of-N multiparty protocol (hegpu_mpc_*): crs = the generator all parties seed alike, rng = the party's own
    def _key_words(self, layout):
        return (1 if layout == MPC_PUBLIC_KEY else self.switch_key_digits()) * 2 * self.Q_prime_size * self.n

    @staticmethod
    def _share_array(shares):
        return (ctypes.c_void_p * max(len(shares), 1))(*[_ptr(s) for s in shares])

    def mpc_public_key_share(self, crs, rng, sk, stream=None):
        import torch
        share = torch.empty(self._key_words(MPC_PUBLIC_KEY), dtype=torch.int64, device="cuda")
        ws = self._kg_ws(OP_MPC_KEY_SHARE)
        self._call("mpc_public_key_share", crs._h, rng._h, _ptr(sk), _ptr(share), _ptr(ws), _ws_bytes(ws),
                   stream=stream)
        return share

    def mpc_relin_key_share_round1(self, crs, rng, sk, stream=None):
        """-> (u, share): u is the party's ephemeral secret, to be handed to round 2 and to nobody else"""
        import torch
        u = torch.empty(self.Q_prime_size * self.n, dtype=torch.int64, device="cuda")
        share = torch.empty(self._key_words(MPC_RELIN_ROUND1), dtype=torch.int64, device="cuda")
        ws = self._kg_ws(OP_MPC_KEY_SHARE)
        self._call("mpc_relin_key_share_round1", crs._h, rng._h, _ptr(sk), _ptr(u), _ptr(share), _ptr(ws),
                   _ws_bytes(ws), stream=stream)
        return u, share

    def mpc_relin_key_share_round2(self, rng, sk, u, round1_sum, stream=None):
        import torch
        share = torch.empty(self._key_words(MPC_RELIN_ROUND1), dtype=torch.int64, device="cuda")
        ws = self._kg_ws(OP_MPC_KEY_SHARE)
        self._call("mpc_relin_key_share_round2", rng._h, _ptr(sk), _ptr(u), _ptr(round1_sum), _ptr(share), _ptr(ws),
                   _ws_bytes(ws), stream=stream)
        return share

    def mpc_galois_key_share(self, crs, rng, sk, galois_elt, stream=None):
        import torch
        share = torch.empty(self._key_words(MPC_GALOIS_KEY), dtype=torch.int64, device="cuda")
        ws = self._kg_ws(OP_MPC_KEY_SHARE)
        self._call("mpc_galois_key_share", crs._h, rng._h, _ptr(sk), galois_elt, _ptr(share), _ptr(ws), _ws_bytes(ws),
                   stream=stream)
        return share

    def mpc_accumulate(self, shares, layout, stream=None):
        import torch
        out = torch.empty(self._key_words(layout), dtype=torch.int64, device="cuda")
        self._call("mpc_accumulate", self._share_array(shares), len(shares), layout, _ptr(out), stream=stream)
        return out

    def mpc_relin_key_finish(self, round2_shares, round1_sum, stream=None):
        import torch
        rk = torch.empty(self._key_words(MPC_RELIN_ROUND1), dtype=torch.int64, device="cuda")
        self._call("mpc_relin_key_finish", self._share_array(round2_shares), len(round2_shares), _ptr(round1_sum),
                   _ptr(rk), stream=stream)
        return rk

    def mpc_ckks_decrypt_share(self, rng, ct, ct_stride, sk, depth=0, batch=1, stream=None):
        import torch
        share = torch.empty(batch * (self.Q_size - depth) * self.n, dtype=torch.int64, device="cuda")
        self._call("mpc_ckks_decrypt_share", rng._h, _ptr(ct), ct_stride, _ptr(sk), depth, _ptr(share), batch,
                   stream=stream)
        return share

    def mpc_ckks_decrypt_merge(self, ct, ct_stride, shares, depth=0, batch=1, stream=None):
        import torch
        plain = torch.empty(batch * (self.Q_size - depth) * self.n, dtype=torch.int64, device="cuda")
        self._call("mpc_ckks_decrypt_merge", _ptr(ct), ct_stride, self._share_array(shares), len(shares), depth,
                   _ptr(plain), batch, stream=stream)
        return plain

    def mpc_bfv_decrypt_share(self, rng, ct, ct_stride, sk, batch=1, stream=None):
        import torch
        share = torch.empty(batch * self.Q_size * self.n, dtype=torch.int64, device="cuda")
        self._call("mpc_bfv_decrypt_share", rng._h, _ptr(ct), ct_stride, _ptr(sk), _ptr(share), batch, stream=stream)
        return share

    def mpc_bfv_decrypt_merge(self, ct, ct_stride, shares, batch=1, stream=None):
        import torch
        plain = torch.empty(batch * self.n, dtype=torch.int64, device="cuda")
        ws = self.workspace(OP_MPC_BFV_DECRYPT_MERGE, 0, batch)
        self._call("mpc_bfv_decrypt_merge", _ptr(ct), ct_stride, self._share_array(shares), len(shares), _ptr(plain),
                   batch, _ptr(ws), _ws_bytes(ws), stream=stream)
        return plain

    # ---- collective refresh (hegpu_mpc_*_refresh_*): crs takes one stream per call, the parties and the coordinator
    # must start from equally advanced generators
    def mpc_ckks_refresh_share(self, crs, rng, ct, ct_stride, sk, depth, mask_bits, batch=1, stream=None):
        """-> share [batch][(Q - depth) + Q][N]: (c1 s_i + NTT(e0 - M_i), -(a s_i) + NTT(e1 + M_i))"""
        import torch
        share = torch.empty(batch * (2 * self.Q_size - depth) * self.n, dtype=torch.int64, device="cuda")
        ws = self.workspace(OP_MPC_REFRESH_SHARE, depth, batch)
        self._call("mpc_ckks_refresh_share", crs._h, rng._h, _ptr(ct), ct_stride, _ptr(sk), depth, mask_bits,
                   _ptr(share), batch, _ptr(ws), _ws_bytes(ws), stream=stream)
        return share

    def mpc_ckks_refresh_merge(self, crs, ct, ct_stride, shares, depth, batch=1, out=None, out_stride=None, stream=None):
        """-> [batch][2][Q][N] at depth 0 (items out_stride apart when `out` is given), the scale unchanged"""
        import torch
        words = 2 * self.Q_size * self.n
        out_stride = words if out_stride is None else out_stride
        if out is None:
            out = torch.empty(max(batch - 1, 0) * out_stride + words, dtype=torch.int64, device="cuda")
        ws = self.workspace(OP_MPC_REFRESH_MERGE, depth, batch)
        self._call("mpc_ckks_refresh_merge", crs._h, _ptr(ct), ct_stride, self._share_array(shares), len(shares), depth,
                   _ptr(out), out_stride, batch, _ptr(ws), _ws_bytes(ws), stream=stream)
        return out

    def mpc_bfv_refresh_share(self, crs, rng, ct, ct_stride, sk, batch=1, stream=None):
        """-> share [batch][2][Q][N], coefficient domain"""
        import torch
        share = torch.empty(batch * 2 * self.Q_size * self.n, dtype=torch.int64, device="cuda")
        ws = self.workspace(OP_MPC_REFRESH_SHARE, 0, batch)
        self._call("mpc_bfv_refresh_share", crs._h, rng._h, _ptr(ct), ct_stride, _ptr(sk), _ptr(share), batch, _ptr(ws),
                   _ws_bytes(ws), stream=stream)
        return share

    def mpc_bfv_refresh_merge(self, crs, ct, ct_stride, shares, batch=1, out=None, out_stride=None, stream=None):
        import torch
        words = 2 * self.Q_size * self.n
        out_stride = words if out_stride is None else out_stride
        if out is None:
            out = torch.empty(max(batch - 1, 0) * out_stride + words, dtype=torch.int64, device="cuda")
        ws = self.workspace(OP_MPC_REFRESH_MERGE, 0, batch)
        self._call("mpc_bfv_refresh_merge", crs._h, _ptr(ct), ct_stride, self._share_array(shares), len(shares),
                   _ptr(out), out_stride, batch, _ptr(ws), _ws_bytes(ws), stream=stream)
        return out


GATE_NAND, GATE_AND, GATE_AND_FIRST_NOT, GATE_NOR, GATE_OR, GATE_XNOR, GATE_XOR, GATE_NOT = range(8)


class Rng:
    """The backend's DRBG handle (ChaCha20 counter-mode streams, csrc/drbg.hpp).  Rng(int): the
    reproducible 64-bit test seed; Rng(bytes of length 32): a full seed; Rng(None): OS entropy."""

    def __init__(self, seed=None):
        self._lib = _lib.load()
        h = ctypes.c_void_p()
        if seed is None:
            _check(self._lib.hegpu_rng_create_from_entropy(ctypes.byref(h)))
        elif isinstance(seed, (bytes, bytearray)):
            assert len(seed) == 32
            _check(self._lib.hegpu_rng_create_seeded(bytes(seed), ctypes.byref(h)))
        else:
            _check(self._lib.hegpu_rng_create(int(seed) & (2**64 - 1), ctypes.byref(h)))
        self._h = h

    def __del__(self):
        try:
            if self._h:
                self._lib.hegpu_rng_destroy(self._h)
                self._h = None
        except Exception:
            pass


class TfheContext(_Handle):
    """HEContext<TFHE> + HELogicOperator<TFHE> over the C ABI (fixed STD128 set)."""

    def __init__(self):
        self._lib = _lib.load()
        h = ctypes.c_void_p()
        _check(self._lib.hegpu_tfhe_context_create(ctypes.byref(h)))
        self._h = h

    def set_option(self, name, value):
        _check(self._lib.hegpu_tfhe_context_set_option(self._h, name.encode(), int(value)))

    def close(self):
        if self._h:
            self._lib.hegpu_tfhe_context_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def int(self, name):
        return int(self._lib.hegpu_tfhe_context_int(self._h, name.encode()))

    @property
    def prime(self):
        return int(self._lib.hegpu_tfhe_prime(self._h))

    def prepare_bootkey(self, boot_key, stream=None):
        import torch
        out = torch.empty(self.int("prepared_bootkey_elems"), dtype=torch.int64, device=boot_key.device)
        self._call("tfhe_prepare_bootkey", _ptr(boot_key), _ptr(out), stream=stream)
        return out

    @staticmethod
    def prepared_is_fp64(prepared):
        """True when the prepared key uses the FP64 blind-rotate layout (real torus32 key)."""
        return int(prepared[0].item()) == 1

    def prepared_format(self, prepared, refresh=False):
        """1 = FP64 layout, 0 = integer layout: the buffer's header word, read after the device has drained
        (hegpu_tfhe_prepared_format; a query -- the blind rotate reads the word itself, on the device)"""
        f = self._lib.hegpu_tfhe_prepared_format(self._h, _ptr(prepared), 1 if refresh else 0)
        if f not in (0, 1):
            raise HEError(f, _lib.load().hegpu_last_error().decode())
        return f

    def gate_precompute(self, gate, out_a, out_b, a1, b1, a2, b2, shape, stream=None):
        self._call("tfhe_gate_precompute", gate, _ptr(out_a), _ptr(out_b), _ptr(a1), _ptr(b1), _ptr(a2), _ptr(b2),
                   shape, stream=stream)

    def bootstrapping(self, in_a, in_b, prepared_bk, out_a, out_b, shape, stream=None):
        self._call("tfhe_bootstrapping", _ptr(in_a), _ptr(in_b), _ptr(prepared_bk), _ptr(out_a), _ptr(out_b), shape,
                   stream=stream)

    def status(self, stream=None):
        """drains the stream; raises HEError(E_INVALID) if a bootstrapping call was handed a buffer that is no prepared key"""
        self._call("tfhe_status", stream=stream)

    def key_switching(self, in_a, in_b, out_a, out_b, ks_a, ks_b, shape, stream=None):
        self._call("tfhe_key_switching", _ptr(in_a), _ptr(in_b), _ptr(out_a), _ptr(out_b), _ptr(ks_a), _ptr(ks_b),
                   shape, stream=stream)

    # ---- front end: keys, bit encryption, decryption, MUX
    def generate_secret_key(self, rng, stream=None):
        import torch
        lwe = torch.empty(self.int("n"), dtype=torch.int32, device="cuda")
        tlwe = torch.empty(self.int("N") * self.int("k"), dtype=torch.int32, device="cuda")
        self._call("tfhe_generate_secret_key", rng._h, _ptr(lwe), _ptr(tlwe), stream=stream)
        return lwe, tlwe

    def generate_bootstrapping_key(self, rng, lwe, tlwe, stream=None):
        """returns (boot key in the reference layout, ks_a, ks_b)"""
        import torch
        bk = torch.empty(self.int("bootkey_elems"), dtype=torch.int64, device="cuda")
        ks_a = torch.empty(self.int("kskey_a_elems"), dtype=torch.int32, device="cuda")
        ks_b = torch.empty(self.int("kskey_b_elems"), dtype=torch.int32, device="cuda")
        ws = torch.empty(self.int("N"), dtype=torch.int64, device="cuda")
        self._call("tfhe_generate_bootstrapping_key", rng._h, _ptr(lwe), _ptr(tlwe), _ptr(bk), _ptr(ks_a), _ptr(ks_b),
                   _ptr(ws), _ws_bytes(ws), stream=stream)
        return bk, ks_a, ks_b

    def encrypt(self, rng, lwe, messages, stream=None):
        import torch
        shape = messages.numel()
        a = torch.empty(shape * self.int("n"), dtype=torch.int32, device="cuda")
        b = torch.empty(shape, dtype=torch.int32, device="cuda")
        self._call("tfhe_encrypt", rng._h, _ptr(lwe), _ptr(messages), shape, _ptr(a), _ptr(b), stream=stream)
        return a, b

    def decrypt_phase(self, lwe, a, b, stream=None):
        import torch
        out = torch.empty(b.numel(), dtype=torch.int32, device="cuda")
        self._call("tfhe_decrypt_phase", _ptr(lwe), _ptr(a), _ptr(b), b.numel(), _ptr(out), stream=stream)
        return out

    def mux(self, a1, b1, a2, b2, ca, cb, out_a, out_b, prepared_bk, ks_a, ks_b, shape, ws, stream=None):
        self._call("tfhe_mux", _ptr(a1), _ptr(b1), _ptr(a2), _ptr(b2), _ptr(ca), _ptr(cb), _ptr(out_a), _ptr(out_b),
                   _ptr(prepared_bk), _ptr(ks_a), _ptr(ks_b), shape, _ptr(ws), _ws_bytes(ws), stream=stream)

    def gate(self, gate, a1, b1, a2, b2, out_a, out_b, prepared_bk, ks_a, ks_b, shape, ws, stream=None):
        self._call("tfhe_gate", gate, _ptr(a1), _ptr(b1), _ptr(a2), _ptr(b2), _ptr(out_a), _ptr(out_b),
                   _ptr(prepared_bk), _ptr(ks_a), _ptr(ks_b), shape, _ptr(ws), _ws_bytes(ws), stream=stream)


LinearTransformPlan = collections.namedtuple("LinearTransformPlan",
                                             "n1 n2 index baby_shifts giant_shifts pre_rotation")


def linear_transform_plan(diag_indices, slots, n1=None, stride=1):
    """Baby-step/giant-step plan of y = M v for a matrix given by its diagonals diag_k[s] = M[s][(s + k) mod slots]
    (host only; the inputs of hegpu_ckks_linear_transform).  `n1` is the baby-step period: diagonal k = j * n1 + i is
    baby step i of giant step j; by default the power of two nearest the square root of the number of diagonals (the
    larger one on a tie), at most 16.  Only the baby steps i and giant steps j that occur are kept.  Returns
      n1, n2         the number of baby / giant rotations (the entry's n1 and n2; n1 is at most the period)
      index          n2 rows of n1 positions in the sorted diagonal list, -1 where the matrix has no such diagonal
      baby_shifts    the occurring i, ascending: column c of index belongs to baby_shifts[c]
      giant_shifts   the occurring j * period, ascending: row r of index belongs to giant_shifts[r]
      pre_rotation   per sorted diagonal, the shift -j * period to rotate its slot vector by before encoding, so that
                     rot(j * period, diag' * rot(i, v)) = diag_k * rot(k, v)
    where a positive shift moves slot s + shift to slot s (rotate_rows; numpy.roll(x, -shift)).  A plan of more than
    16 giant steps is refused: choose a larger period.
    `stride`: every diagonal index is a multiple of it (a group of FFT stages, encoding_transform_factors) and the plan
    is made over k / stride: diagonal k = stride * (j * n1 + i), baby shifts stride * i, giant shifts stride * j * n1,
    all modulo slots.  Without it such a matrix has the single baby step 0 and one giant step per diagonal."""
    ks = sorted({int(k) % slots for k in diag_indices})
    if not ks:
        raise ValueError("a linear transform needs at least one diagonal")
    if stride < 1 or any(k % stride for k in ks):
        raise ValueError("every diagonal index is a multiple of the stride")
    if n1 is None:
        root = len(ks) ** 0.5
        n1 = min((1, 2, 4, 8, 16), key=lambda p: (abs(p - root), -p))
    if not 1 <= n1 <= 16:
        raise ValueError("the baby-step period lies in [1, 16]")
    qs = [k // stride for k in ks]
    baby = sorted({q % n1 for q in qs})
    giant = sorted({q // n1 for q in qs})
    if len(giant) > 16:
        raise ValueError(f"{len(giant)} giant steps, at most 16 fit one transform: choose a larger period")
    index = [[-1] * len(baby) for _ in giant]
    for pos, q in enumerate(qs):
        index[giant.index(q // n1)][baby.index(q % n1)] = pos
    return LinearTransformPlan(len(baby), len(giant), index, [stride * i for i in baby], [stride * j * n1 for j in giant],
                               [-stride * (q // n1) * n1 for q in qs])


GiantStepChain = collections.namedtuple("GiantStepChain", "parent link_shifts")


def giant_step_chain(giant_shifts, slots):
    """The chain of a plan's giant steps (host only; hegpu_giant_step_chain): a Horner fold over the signed shifts.  The
    non-negative shifts, ascending, each hang on the one before; the negative ones, from the one nearest zero outwards,
    likewise, the first of them on the zero shift if there is one.  Returns
      parent         per giant step the term it is folded into, -1 for a root
      link_shifts    per giant step its shift minus its parent's, in [0, slots); for a root its own shift
    the giant_parent of Context.ckks_linear_transform and the rotations of its links.  The links a term crosses add up to
    its giant shift, so linear_transform_plan's pre_rotation stays valid."""
    shifts = [int(s) for s in giant_shifts]
    n2 = len(shifts)
    arr = (ctypes.c_int * max(n2, 1))(*shifts)
    parent, links = (ctypes.c_int * max(n2, 1))(), (ctypes.c_int * max(n2, 1))()
    _check(_lib.load().hegpu_giant_step_chain(arr, n2, int(slots), parent, links))
    return GiantStepChain(list(parent)[:n2], list(links)[:n2])


def chained_giant_steps(giant_shifts, n, galois_key):
    """The giant-step arguments of a chained transform at degree n: (keys, elts, parent, link_shifts) with the keys of
    the links from galois_key(elt) -> device key (None where a link does not rotate)."""
    chain = giant_step_chain(giant_shifts, n // 2)
    elts = [steps_to_galois_elt(s, n, 5) if s else 0 for s in chain.link_shifts]
    return [galois_key(e) if e else None for e in elts], elts, chain.parent, chain.link_shifts


EncodingTransformPiece = collections.namedtuple("EncodingTransformPiece", "stride stages offsets diagonals")


def encoding_transform_factors(n, inverse, pieces):
    """The factors of the CKKS encoder's special FFT in diagonal form (host only; hegpu_encoding_transform_shape /
    _fill): `pieces` groups of consecutive radix-2 stages in the order they are applied.  inverse=False: the SlotToCoeff
    factors, their product is U B (U[j][k] = zeta^(5^j k), B the bit reversal); inverse=True: the CoeffToSlot factors,
    their product is 1/2 B U^-1.  Per group: the stride (every offset is a multiple of it), the number of stages, the
    signed diagonal offsets and a complex array [len(offsets)][n / 2] with diagonals[d][t] = M[t][(t + offsets[d]) mod
    n / 2]."""
    import numpy as np
    lib = _lib.load()
    strides, stages, counts = ((ctypes.c_int * pieces)() for _ in range(3))
    _check(lib.hegpu_encoding_transform_shape(n, int(bool(inverse)), pieces, strides, stages, counts))
    out = []
    for p in range(pieces):
        offsets = (ctypes.c_int * counts[p])()
        values = np.empty((counts[p], n // 2), dtype=np.complex128)
        _check(lib.hegpu_encoding_transform_fill(n, int(bool(inverse)), pieces, p, counts[p], offsets,
                                                 values.ctypes.data))
        out.append(EncodingTransformPiece(strides[p], stages[p], list(offsets), values))
    return out


MONOMIAL, CHEBYSHEV = 0, 1
POLY_POWER, POLY_LEAF, POLY_COMBINE = 0, 1, 2
POLY_TAIL_NONE, POLY_TAIL_ONE = -1, -2
PolyEvalPlan = collections.namedtuple("PolyEvalPlan", "steps level scale out_limbs")


def _primes_array(primes):
    """primes as the (uint64 array, count) pair the host-only planners end their arguments with"""
    pr = [int(p) for p in primes]
    return (ctypes.c_uint64 * max(len(pr), 1))(*pr), len(pr)


def _step_plan(size, fill, *args):
    """One _size / _fill pair of the C ABI over the arguments the two share, as a PolyEvalPlan."""
    count = ctypes.c_int(0)
    _check(size(*args, ctypes.byref(count)))
    steps = (_lib.PolyStep * count.value)()
    _check(fill(*args, steps, count.value))
    last = steps[count.value - 1]
    return PolyEvalPlan(steps, last.level, last.scale, last.level + 1 + last.rescale_after)


def poly_eval_plan(basis, coeffs, level, scale, target_scale, primes, max_deg=None, lead=True):
    """The evaluation order of sum_i coeffs[i] b_i(x) on a CKKS ciphertext (host only; hegpu_poly_eval_plan_size / _fill),
    b_i = x^i (MONOMIAL) or T_i (CHEBYSHEV, x in [-1, 1]): the reference's baby-step/giant-step schedule.  level / scale:
    of the input ciphertext (level = Q - 1 - depth); primes: the context's q_0 ...; max_deg / lead: the reference's
    Polynomial::max_deg_ (default: the degree) and lead_.  Returns
      steps      a ctypes array of hegpu_poly_step (include/hegpu.h): kind, dst, a, b, c, level, mul_level, rescale_first,
                 rescale_after, n_terms, term_reg, scale, tail_const, w0, w
      level      of the result (its depth is Q - 1 - level)
      scale      of the result
      out_limbs  limbs per part the output buffer of Context.ckks_poly_eval needs (one more than level + 1 when the last
                 step rescales)"""
    lib = _lib.load()
    c = np.ascontiguousarray(np.asarray(coeffs, dtype=np.complex128).reshape(-1))
    arr, n_primes = _primes_array(primes)
    md = len(c) - 1 if max_deg is None else int(max_deg)
    return _step_plan(lib.hegpu_poly_eval_plan_size, lib.hegpu_poly_eval_plan_fill, int(basis), c.ctypes.data, len(c), md,
                      int(bool(lead)), int(level), float(scale), float(target_scale), arr, n_primes)


def eval_mod_plan(K, degree, double_angle, level, scale, target_scale, primes):
    """EvalMod of CKKS bootstrapping as a plan for Context.ckks_poly_eval (host only; hegpu_eval_mod_plan_size / _fill).  The
    input holds u in [-1, 1] with K u = I + eps, I an integer below K in magnitude; the plan evaluates the degree-`degree`
    Chebyshev interpolant of (1 / 2 pi)^(1 / 2^r) cos(2 pi (K u - 1/4) / 2^r), r = double_angle, and then r double-angle
    steps, which leaves sin(2 pi eps) / 2 pi at target_scale.  Returns a PolyEvalPlan like poly_eval_plan."""
    lib = _lib.load()
    arr, n_primes = _primes_array(primes)
    return _step_plan(lib.hegpu_eval_mod_plan_size, lib.hegpu_eval_mod_plan_fill, int(K), int(degree), int(double_angle),
                      int(level), float(scale), float(target_scale), arr, n_primes)


class _RefreshPlan:
    """What the plans of the refreshes share: c is the C struct; the other attributes are c's fields, arrays cut to their
    piece counts."""

    def __init__(self, c):
        self.c = c
        for name, _t in c._fields_:
            setattr(self, name, getattr(c, name))
        self.cts_scale, self.cts_label = list(c.cts_scale)[:c.cts_pieces], list(c.cts_label)[:c.cts_pieces]
        self.stc_scale, self.stc_label = list(c.stc_scale)[:c.stc_pieces], list(c.stc_label)[:c.stc_pieces]


class BootstrapPlan(_RefreshPlan):
    """The plan of the CKKS refresh (bootstrap_plan): c is the hegpu_bootstrap_plan, eval_mod the EvalMod PolyEvalPlan it
    names; the other attributes are c's fields, arrays cut to their piece counts."""

    def __init__(self, c, eval_mod):
        super().__init__(c)
        self.eval_mod, self.k1 = eval_mod, int(c.k1)


def bootstrap_plan(primes, scale, cts_level, cts_pieces=3, stc_pieces=3, message_ratio=256.0, K=16, sine_degree=30,
                   double_angle=3, eval_level=-1, stc_level=-1):
    """Every level and scale label of the CKKS refresh (host only; hegpu_bootstrap_plan_fill) and the EvalMod plan that goes
    with it.  primes: q_0 ...; scale: of the ciphertext to refresh; cts_level: the level the modulus raise goes to.  The
    defaults are the reference's EvalModConfig(level_start).  Returns a BootstrapPlan: k1 (the integer the q_0 limbs are
    multiplied by), raise_scale, cts_scale / stc_scale (what each factor's diagonals are encoded at), eval_level, stc_level,
    out_level, out_scale, eval_mod."""
    lib = _lib.load()
    arr, n_primes = _primes_array(primes)
    cfg = _lib.BootstrapConfig(float(scale), float(message_ratio), int(K), int(sine_degree), int(double_angle), int(cts_level),
                               int(cts_pieces), int(eval_level), int(stc_level), int(stc_pieces))
    c = _lib.BootstrapPlan()
    _check(lib.hegpu_bootstrap_plan_fill(ctypes.byref(cfg), arr, n_primes, ctypes.byref(c)))
    return BootstrapPlan(c, eval_mod_plan(c.K, c.sine_degree, c.double_angle, c.eval_level, c.eval_in_scale,
                                          c.eval_target_scale, arr[:n_primes]))


def eval_trig_plan(K, degree, double_angle, phase, amplitude, offset, level, scale, target_scale, primes):
    """offset + amplitude cos(2 pi (K u - phase)) as a plan for Context.ckks_poly_eval (host only; hegpu_eval_trig_plan_size /
    _fill): the interpolant of amplitude^(1 / 2^r) cos(2 pi (K u - phase) / 2^r), r double-angle steps, the last one's tail
    constant amplitude - offset.  eval_mod_plan is (1/4, 1 / 2 pi, 0).  Returns a PolyEvalPlan like poly_eval_plan."""
    lib = _lib.load()
    arr, n_primes = _primes_array(primes)
    return _step_plan(lib.hegpu_eval_trig_plan_size, lib.hegpu_eval_trig_plan_fill, int(K), int(degree), int(double_angle),
                      float(phase), float(amplitude), float(offset), int(level), float(scale), float(target_scale), arr, n_primes)


# (ratio, phase, amplitude, offset) of the slim family: alpha + A cos(2 pi (a / ratio - phi)); ratio None: the caller's
SLIM_FUNCTIONS = {
    "slim": (None, 1 / 4, 1 / (2 * np.pi), 0.0),
    "bit": (2.0, 1 / 2, 1 / 2, 1 / 2),
    "and": (3.0, 2 / 3, 2 / 3, 1 / 3),
    "or": (3.0, 1 / 2, 2 / 3, 2 / 3),
    "xor": (3.0, 1 / 3, 2 / 3, 1 / 3),
    "nand": (3.0, 1 / 6, 2 / 3, 2 / 3),
    "nor": (3.0, 0.0, 2 / 3, 1 / 3),
    "xnor": (3.0, 5 / 6, 2 / 3, 2 / 3),
}


class SlimBootstrapPlan(_RefreshPlan):
    """The plan of a slim, bit or gate refresh (slim_bootstrap_plan): c is the hegpu_slim_bootstrap_plan, trig the
    PolyEvalPlan it names; the other attributes are c's fields, arrays cut to their piece counts."""

    def __init__(self, c, trig):
        super().__init__(c)
        self.trig = trig


def slim_bootstrap_plan(primes, scale, cts_level, function="slim", cts_pieces=3, stc_pieces=3, ratio=256.0, K=12, degree=30,
                        double_angle=3):
    """Every level and scale label of a slim, bit or gate refresh (host only; hegpu_slim_bootstrap_plan_fill) and the trig
    plan that goes with it.  primes: q_0 ...; scale: of the ciphertext to refresh, which sits at level stc_pieces;
    cts_level: the level the modulus raise goes to; function: a key of SLIM_FUNCTIONS or a (ratio, phase, amplitude, offset)
    tuple; ratio: for "slim" only.  Returns a SlimBootstrapPlan: in_level, stc_scale / cts_scale (what each factor's diagonals
    are encoded at), raise_scale, eval_level, out_level, out_scale, trig."""
    lib = _lib.load()
    arr, n_primes = _primes_array(primes)
    arithmetic = function == "slim"
    rho, phase, amplitude, offset = SLIM_FUNCTIONS[function] if isinstance(function, str) else function
    cfg = _lib.SlimBootstrapConfig(float(scale), float(ratio if rho is None else rho), float(phase), float(amplitude),
                                   float(offset), int(K), int(degree), int(double_angle), int(cts_level), int(cts_pieces),
                                   int(stc_pieces), int(arithmetic), 0)
    c = _lib.SlimBootstrapPlan()
    _check(lib.hegpu_slim_bootstrap_plan_fill(ctypes.byref(cfg), arr, n_primes, ctypes.byref(c)))
    return SlimBootstrapPlan(c, eval_trig_plan(c.K, c.degree, c.double_angle, c.phase, c.amplitude, c.offset, c.eval_level,
                                               c.eval_in_scale, c.eval_target_scale, arr[:n_primes]))


def ks_launch_forms():
    """measurement seam: (natural, wide, split) launches of the fused row pass + inner product so far in this process"""
    c = (ctypes.c_uint64 * 3)()
    _lib.load().hegpu_probe_ks_launch_forms(c)
    return tuple(int(x) for x in c)


def steps_to_galois_elt(steps, n, group_order):
    return int(_lib.load().hegpu_steps_to_galois_elt(steps, n, group_order))
