"""not-gpu: the host side of awq_mla_kv_store -- the refusals that precede any launch, and the presence of the name."""
import ctypes
import os

import pytest

from llm_awq_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_SHAPE, ERR_DTYPE, ERR_ALIGN, ERR_NULL = -4, -3, -5, -6


def test_name_is_declared_exported_and_bound():
    from llm_awq_amd import ops
    header = open(os.path.join(ROOT, "include", "awq_cdna4.h")).read()
    n = "awq_mla_kv_store"
    assert n + "(" in header and hasattr(ctypes.CDLL(_capi.LIB_PATH), n) and n in _capi.SIGNATURES and callable(ops.mla_kv_store)
    assert _capi.lib().awq_abi_version() == 1


def _refused(fn, args, kw):
    """fn on valid host pointers with kw's fields replaced ("p+n": the aligned pointer + n bytes); nothing is launched."""
    raw = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(raw) + 15) & ~15
    return fn(*args(p, **{k: (p + int(v[2:] or 0) if isinstance(v, str) else v) for k, v in kw.items()}))


def store_args(p, **kw):
    a = dict(kv=p, qpe=p, qabs=p, cache=p, table=None, cu=p, lens=p, freqs=p, gamma=p, eps=1e-6, B=2, H=16, T=4, sq=2, P=4096, il=1, outer=2,
             rows=128, pps=0, bt_rs=0, kv_rs=576, q_ts=16 * 192, q_hs=192, c_os=128 * 576, c_rs=576, dtype=1)
    a.update(kw)
    return [a[k] for k in ("kv", "qpe", "qabs", "cache", "table", "cu", "lens", "freqs", "gamma", "eps", "B", "H", "T", "sq", "P", "il", "outer", "rows",
                           "pps", "bt_rs", "kv_rs", "q_ts", "q_hs", "c_os", "c_rs", "dtype")] + [None]


@pytest.mark.parametrize("kw, code", [
    (dict(kv=None), ERR_NULL), (dict(gamma=None), ERR_NULL), (dict(freqs=None), ERR_NULL), (dict(dtype=7), ERR_DTYPE),
    (dict(H=129), ERR_SHAPE), (dict(il=2), ERR_SHAPE), (dict(kv_rs=512), ERR_SHAPE), (dict(q_hs=32), ERR_SHAPE), (dict(eps=-1.0), ERR_SHAPE),
    (dict(table="p", outer=4, rows=100, pps=2, bt_rs=2), ERR_SHAPE),
    (dict(kv="p+4"), ERR_ALIGN), (dict(gamma="p+4"), ERR_ALIGN), (dict(kv_rs=580), ERR_ALIGN), (dict(cu="p+1"), ERR_ALIGN),
])
def test_store_refuses_before_any_launch(kw, code):
    assert _refused(_capi.lib().awq_mla_kv_store, store_args, kw) == code
