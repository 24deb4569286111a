"""Shared-prefix decode without a GPU: the exports, the plan and workspace formulas, every argument check of the new C entries, the page
allocator's reference counts and `fork`, the bookkeeping of `PrefixGroups`, and the soundness of the needle batches of
tests/attn_shared_cases.py -- the list tests/test_gpu_attention_shared.py runs through the kernels -- against the torch restatement of
the contract (tests/attn_shared_oracle.py) and each of its mutants."""
import ctypes
import inspect

import pytest
import torch

from llm_awq_amd import _capi, ops
from llm_awq_amd.paged_kv import PagePoolExhausted, PageTable, PrefixGroups
from tests import attn_shared_cases as C
from tests import attn_shared_oracle as O

AWQ_OK, AWQ_ERR_DTYPE, AWQ_ERR_SHAPE, AWQ_ERR_ALIGN, AWQ_ERR_NULL, AWQ_ERR_WORKSPACE = 0, -3, -4, -5, -6, -7
SYMBOLS = ("awq_attn_kvcache_shared_plan", "awq_attn_kvcache_shared_workspace_bytes", "awq_attn_kvcache_paged_shared",
           "awq_attn_kvcache_paged_shared_kv8", "awq_kv_page_copy", "awq_kv_page_copy_fp8")


def _bits(t):
    return t.view(torch.int16)


def test_library_and_ops_export_the_shared_surface():
    L = _capi.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in _capi.SIGNATURES, name
    assert len(_capi.SIGNATURES["awq_attn_kvcache_paged_shared"][1]) == len(_capi.SIGNATURES["awq_attn_kvcache_paged"][1]) + 7
    assert len(_capi.SIGNATURES["awq_attn_kvcache_paged_shared_kv8"][1]) == len(_capi.SIGNATURES["awq_attn_kvcache_paged_kv8"][1]) + 7
    assert list(inspect.signature(ops.attn_kvcache_paged_shared).parameters) == [
        "q", "k_pool", "v_pool", "block_table", "seqlens_k", "max_seqlen_k", "group_members", "group_prefix", "seq_prefix", "max_prefix",
        "seqlen_offset", "softmax_scale", "causal", "k_scale", "v_scale"]
    assert list(inspect.signature(ops.kv_page_copy).parameters) == ["k_pool", "v_pool", "src_pages", "dst_pages", "k_scale", "v_scale"]
    q = torch.zeros(2, 1, 8, 128, dtype=torch.float16)
    pool = torch.zeros(4, 64, 2, 128, dtype=torch.float16)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)  # noqa: E731
    with pytest.raises(RuntimeError, match="GPU"):
        ops.attn_kvcache_paged_shared(q, pool, pool, i32(2, 4), i32(2), 256, i32(1, 2), i32(1), i32(2), 64)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.kv_page_copy(pool, pool, i32(1), i32(1))


# ------------------------------------------------------------------------------------------------------------------------
# plan and workspace
# ------------------------------------------------------------------------------------------------------------------------
def test_plan_is_the_kvcache_rule_twice_and_the_workspace_holds_both():
    L = _capi.lib()
    try:
        for B, H, Hkv, Dh, Sq, mp, bound in ((32, 32, 8, 128, 1, 32768, 33024), (32, 32, 8, 128, 1, 2048, 2304), (4, 8, 2, 64, 3, 64, 64),
                                             (1, 8, 8, 128, 2, 8192, 131072), (7, 8, 2, 64, 1, 256, 384)):
            sp, cp, ss, cs = ops.attn_kvcache_shared_plan(B, H, Hkv, Dh, Sq, mp, bound)
            assert (sp, cp) == ops.attn_kvcache_plan(B, H, Hkv, Dh, Sq, mp) and (ss, cs) == ops.attn_kvcache_plan(B, H, Hkv, Dh, Sq, bound)
            assert sp * cp >= mp and ss * cs >= bound and cp % 64 == 0 and cs % 64 == 0
            assert L.awq_attn_kvcache_shared_workspace_bytes(B, H, Hkv, Dh, Sq, mp, bound) == B * H * Sq * (sp + ss) * (Dh + 2) * 4
        assert ops.attn_kvcache_shared_plan(32, 32, 8, 128, 1, 2048, 2304) == (2, 1024, 3, 1024)
        for chunk in (64, 256):  # the knob forces both chunks
            _capi.tune(attn_splitkv_chunk=chunk)
            assert ops.attn_kvcache_shared_plan(7, 8, 2, 64, 1, 256, 384) == O.plan(256, 384, chunk)
            sp, _, ss, _ = O.plan(256, 384, chunk)
            assert L.awq_attn_kvcache_shared_workspace_bytes(7, 8, 2, 64, 1, 256, 384) == 7 * 8 * (sp + ss) * 66 * 4
    finally:
        _capi.tune(attn_splitkv_chunk=0)
    i = ctypes.c_int(0)
    r = ctypes.byref(i)
    for bad in (dict(mp=0), dict(mp=32), dict(mp=100), dict(mp=448), dict(mp=-64), dict(B=0), dict(Dh=96), dict(H=6, Hkv=4), dict(Sq=33), dict(bound=0)):
        a = dict(dict(B=2, H=8, Hkv=2, Dh=128, Sq=1, mp=128, bound=384), **bad)
        args = (a["B"], a["H"], a["Hkv"], a["Dh"], a["Sq"], a["mp"], a["bound"])
        assert L.awq_attn_kvcache_shared_plan(*args, r, r, r, r) == AWQ_ERR_SHAPE, bad
        assert L.awq_attn_kvcache_shared_workspace_bytes(*args) == 0, bad
    assert L.awq_attn_kvcache_shared_plan(2, 8, 2, 128, 1, 128, 384, None, r, r, r) == AWQ_ERR_NULL


# ------------------------------------------------------------------------------------------------------------------------
# argument validation: every code, no GPU call
# ------------------------------------------------------------------------------------------------------------------------
def _p16():
    buf = (ctypes.c_char * 8192)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


ATTN_OK = dict(B=2, Sq=1, off=1, bound=4096, pages=40, ps=256, pps=16, trs=20, H=8, Hkv=2, Dh=128, qbs=1024, qrs=1024, kps=256 * 256, krs=256,
               vps=256 * 256, vrs=256, ksps=256 * 2, ksrs=2, vsps=256 * 2, vsrs=2, scale=0.1, causal=1, dtype=0, ng=3, cap=4, mrs=6, mp=1024)


def _attn(p, kv8=False, **kw):
    """The workspace stays NULL unless a test gives one, so even a call that passes every other check launches nothing."""
    a = dict(ATTN_OK, q=p, k=p, v=p, ks=p, vs=p, out=p, bt=p, lens=p, gm=p, gp=p, sp=p, ws=None, wsb=0)
    a.update(kw)
    L = _capi.lib()
    head = (a["bt"], a["B"], a["Sq"], a["lens"], a["off"], a["bound"], a["pages"], a["ps"], a["pps"], a["trs"], a["H"], a["Hkv"], a["Dh"], a["qbs"],
            a["qrs"], a["kps"], a["krs"], a["vps"], a["vrs"])
    tail = (a["scale"], a["causal"], a["dtype"], a["gm"], a["gp"], a["sp"], a["ng"], a["cap"], a["mrs"], a["mp"], a["ws"], a["wsb"], None)
    if kv8:
        return L.awq_attn_kvcache_paged_shared_kv8(a["q"], a["k"], a["v"], a["ks"], a["vs"], a["out"], *head, a["ksps"], a["ksrs"], a["vsps"],
                                                   a["vsrs"], *tail)
    return L.awq_attn_kvcache_paged_shared(a["q"], a["k"], a["v"], a["out"], *head, *tail)


@pytest.mark.parametrize("kv8", [False, True], ids=["T", "kv8"])
def test_shared_argument_validation_returns_codes_without_launch(kv8):
    buf, p = _p16()
    # the codes of awq_attn_kvcache_paged ..
    for bad in (dict(ps=0), dict(ps=32), dict(ps=96), dict(pages=0), dict(pps=0), dict(trs=15), dict(bound=4097), dict(bound=0), dict(off=-1),
                dict(Dh=96), dict(H=6, Hkv=4), dict(B=0), dict(Sq=0), dict(Sq=33), dict(qrs=512), dict(krs=128), dict(vrs=128), dict(qbs=-8),
                dict(kps=-256), dict(vps=-256)):
        assert _attn(p, kv8, **bad) == AWQ_ERR_SHAPE, bad
    # .. and those of the group arrays: num_groups, group_cap, the row stride, the 128 rows of the tile, max_prefix
    for bad in (dict(ng=0), dict(ng=-1), dict(cap=0), dict(cap=-3), dict(mrs=3), dict(cap=33), dict(cap=9, Sq=4, mrs=9), dict(mp=0), dict(mp=32),
                dict(mp=1000), dict(mp=4160), dict(mp=-64)):
        assert _attn(p, kv8, **bad) == AWQ_ERR_SHAPE, bad
    assert _attn(p, kv8) == AWQ_ERR_WORKSPACE               # everything else is in order
    assert _attn(p, kv8, cap=32, mrs=32) == AWQ_ERR_WORKSPACE and _attn(p, kv8, cap=8, Sq=4, mrs=8) == AWQ_ERR_WORKSPACE   # exactly 128 rows
    assert _attn(p, kv8, mp=64) == AWQ_ERR_WORKSPACE and _attn(p, kv8, mp=4096) == AWQ_ERR_WORKSPACE
    assert _attn(p, kv8, dtype=2) == AWQ_ERR_DTYPE
    for name in ("q", "k", "v", "out", "bt", "lens", "gm", "gp", "sp") + (("ks", "vs") if kv8 else ()):
        assert _attn(p, kv8, **{name: None}) == AWQ_ERR_NULL, name
    for name in ("q", "k", "v", "out"):
        assert _attn(p, kv8, **{name: p + 2}) == AWQ_ERR_ALIGN, name
    for name in ("bt", "lens", "gm", "gp", "sp"):
        assert _attn(p, kv8, **{name: p + 2}) == AWQ_ERR_ALIGN, name
        assert _attn(p, kv8, **{name: p + 4}) == AWQ_ERR_WORKSPACE, name   # four bytes are enough
    need = _capi.lib().awq_attn_kvcache_shared_workspace_bytes(2, 8, 2, 128, 1, 1024, 4096)
    assert need > _capi.lib().awq_attn_kvcache_workspace_bytes(2, 8, 2, 128, 1, 4096) > 0
    assert _attn(p, kv8, ws=p, wsb=need - 1) == AWQ_ERR_WORKSPACE and _attn(p, kv8, ws=p + 4, wsb=need) == AWQ_ERR_ALIGN


@pytest.mark.parametrize("fp8", [False, True], ids=["T", "fp8"])
def test_page_copy_argument_validation_returns_codes_without_launch(fp8):
    """Every call here is refused: a call that passed would launch, and there is no GPU."""
    buf, p = _p16()
    L = _capi.lib()
    ok = dict(k=p, v=p, ks=p, vs=p, src=p, dst=p, n=2, pages=9, ps=64, Hkv=2, Dh=128, kps=64 * 256, krs=256, vps=64 * 256, vrs=256, ksps=128, ksrs=2,
              vsps=128, vsrs=2)

    def call(**kw):
        a = dict(ok, **kw)
        tail = (a["src"], a["dst"], a["n"], a["pages"], a["ps"], a["Hkv"], a["Dh"], a["kps"], a["krs"], a["vps"], a["vrs"])
        if fp8:
            return L.awq_kv_page_copy_fp8(a["k"], a["v"], a["ks"], a["vs"], *tail, a["ksps"], a["ksrs"], a["vsps"], a["vsrs"], None)
        return L.awq_kv_page_copy(a["k"], a["v"], *tail, None)
    for bad in (dict(n=0), dict(n=-1), dict(pages=0), dict(ps=0), dict(ps=32), dict(ps=100), dict(Hkv=0), dict(Dh=96), dict(krs=128), dict(vrs=128),
                dict(kps=-256), dict(vps=-256)) + ((dict(ksrs=1), dict(vsrs=1), dict(ksps=-2), dict(vsps=-2)) if fp8 else ()):
        assert call(**bad) == AWQ_ERR_SHAPE, bad
    for name in ("k", "v", "src", "dst") + (("ks", "vs") if fp8 else ()):
        assert call(**{name: None}) == AWQ_ERR_NULL, name
    for name in ("k", "v"):
        assert call(**{name: p + 4}) == AWQ_ERR_ALIGN, name
    assert call(src=p + 2) == AWQ_ERR_ALIGN and call(dst=p + 2) == AWQ_ERR_ALIGN
    if fp8:
        assert call(ks=p + 2) == AWQ_ERR_ALIGN and call(vs=p + 2) == AWQ_ERR_ALIGN
        for name, val in (("kps", 64 * 256 + 8), ("krs", 264), ("vps", 64 * 256 + 8), ("vrs", 264)):  # strides in codes: multiples of 16
            assert call(**{name: val}) == AWQ_ERR_ALIGN, name
    for name, val in (("kps", 64 * 256 + 4), ("krs", 260), ("vps", 64 * 256 + 4), ("vrs", 260)):
        assert call(**{name: val}) == AWQ_ERR_ALIGN, name


# ------------------------------------------------------------------------------------------------------------------------
# PageTable.fork and the reference counts
# ------------------------------------------------------------------------------------------------------------------------
def test_fork_shares_whole_pages_and_copies_the_tail():
    t = PageTable(num_pages=12, page_size=64, max_batch=4, pages_per_seq=5, device="cpu")
    ptr = t.table.data_ptr()
    assert t.reserve(0, 200) == (0, 1, 2, 3) and all(t.refcount(p) == 1 for p in range(4)) and t.refcount(4) == 0
    pair = t.fork(0, 1, 150)                                # two whole pages and a tail of 22 tokens
    assert pair == (2, 4) and t.pages(1) == (0, 1, 4) and t.table[1].tolist() == [0, 1, 4, 0, 0]
    assert [t.refcount(p) for p in range(5)] == [2, 2, 1, 1, 1] and t.free_pages == 7
    assert t.fork(0, 2, 128) is None and t.pages(2) == (0, 1) and t.refcount(0) == 3 and t.free_pages == 7   # whole pages only: nothing to copy
    assert t.common_prefix((0, 1, 2)) == 128 and t.common_prefix((0, 1)) == 128 and t.common_prefix((0,)) == 256 and t.common_prefix(()) == 0
    assert t.reserve(1, 193) == (5,) and t.pages(1) == (0, 1, 4, 5)   # a forked slot grows behind its tail page
    assert t.reserve(2, 129) == (6,) and t.common_prefix((1, 2)) == 128
    # release: a shared page goes back only when its last holder lets go; the return value counts what THIS slot let go of
    assert t.release(0) == 4 and t.free_pages == 7 and [t.refcount(p) for p in range(4)] == [2, 2, 0, 0] and not t.table[0].any()
    assert t.release(1) == 4 and t.free_pages == 9 and t.refcount(0) == 1
    assert t.release(2) == 3 and t.free_pages == 12 and all(t.refcount(p) == 0 for p in range(12))
    assert sorted(t._free) == list(range(12)) and t.table.data_ptr() == ptr and not t.table.any()
    # refusals change nothing
    t.reserve(0, 100)
    t.reserve(3, 10)
    for bad, what in (((0, 3, 64), "hold nothing"), ((0, 0, 64), "hold nothing"), ((0, 1, 129), "pages"), ((0, 1, 0), "pages")):
        with pytest.raises(ValueError, match=what):
            t.fork(*bad)
    assert t.pages(1) == () and t.free_pages == 9
    small = PageTable(num_pages=2, page_size=64, max_batch=2, pages_per_seq=2, device="cpu")
    small.reserve(0, 100)
    with pytest.raises(PagePoolExhausted, match="tail"):
        small.fork(0, 1, 100)
    assert small.pages(1) == () and small.refcount(0) == 1 and small.fork(0, 1, 64) is None and small.refcount(0) == 2


def test_release_before_on_shared_pages_and_fork_refuses_a_released_head():
    t = PageTable(num_pages=8, page_size=64, max_batch=3, pages_per_seq=4, device="cpu")
    t.reserve(0, 256)
    assert t.fork(0, 1, 192) is None and t.free_pages == 4
    assert t.release_before(0, 130) == 2 and t.free_pages == 4          # slot 1 still holds pages 0 and 1
    assert t.pages(0) == (2, 3) and t.table[0].tolist() == [0, 0, 2, 3] and t.table[1].tolist() == [0, 1, 2, 0]
    assert [t.refcount(p) for p in range(4)] == [1, 1, 2, 1]
    with pytest.raises(ValueError, match="release_before"):
        t.fork(0, 2, 192)
    assert t.common_prefix((0, 1)) == 0                                   # the head of slot 0 is gone
    assert t.release_before(1, 128) == 2 and t.free_pages == 6            # the last holder: now they are free
    assert t.release(1) == 1 and t.free_pages == 6 and t.release(0) == 2 and t.free_pages == 8
    assert all(t.refcount(p) == 0 for p in range(8))


def test_pages_held_by_32_samples_of_a_32768_token_prompt():
    ps, prompt, own = 256, 32768, 256
    t = PageTable(num_pages=32 * (prompt + own) // ps, page_size=ps, max_batch=32, pages_per_seq=(prompt + own) // ps, device="cpu")
    t.reserve(0, prompt)
    for s in range(1, 32):
        assert t.fork(0, s, prompt) is None
    for s in range(32):
        t.reserve(s, prompt + own)
    assert t.num_pages - t.free_pages == prompt // ps + 32 * own // ps   # 160 pages against 4128 without fork
    assert t.common_prefix(range(32)) == prompt


# ------------------------------------------------------------------------------------------------------------------------
# PrefixGroups
# ------------------------------------------------------------------------------------------------------------------------
def test_prefix_groups_keep_the_three_arrays_consistent_in_place():
    g = PrefixGroups(num_groups=3, group_cap=4, max_batch=8, max_prefix=256, device="cpu")
    ptrs = [t.data_ptr() for t in (g.group_members, g.group_prefix, g.seq_prefix)]
    assert g.group_members.dtype == g.group_prefix.dtype == g.seq_prefix.dtype == torch.int32
    assert (g.group_members == -1).all() and not g.group_prefix.any() and not g.seq_prefix.any()
    g.set(0, (5, 1, 3), 192)
    g.set(2, (7,), 64)
    assert g.group_members.tolist() == [[5, 1, 3, -1], [-1] * 4, [7, -1, -1, -1]] and g.group_prefix.tolist() == [192, 0, 64]
    assert g.seq_prefix.tolist() == [0, 192, 0, 192, 0, 192, 0, 64] and g.members(0) == (5, 1, 3) and g.group_of(3) == 0 and g.group_of(0) is None
    g.set(0, (1, 3, 6), 128)                                   # replaces the group: slot 5 is ungrouped again
    assert g.group_members[0].tolist() == [1, 3, 6, -1] and g.seq_prefix.tolist() == [0, 128, 0, 128, 0, 0, 128, 64]
    assert g.remove(1) == 0 and g.group_members[0].tolist() == [3, 6, -1, -1] and g.seq_prefix[1] == 0 and g.remove(1) is None
    assert g.remove(7) == 2 and g.group_prefix.tolist() == [128, 0, 0] and (g.group_members[2] == -1).all()
    g.clear(0)
    assert (g.group_members == -1).all() and not g.group_prefix.any() and not g.seq_prefix.any()
    assert ptrs == [t.data_ptr() for t in (g.group_members, g.group_prefix, g.seq_prefix)]
    g.set(1, (0, 2), 256)
    for bad in (dict(slots=(), n=64), dict(slots=(1, 2, 3, 4, 5), n=64), dict(slots=(1, 1), n=64), dict(slots=(8,), n=64), dict(slots=(1,), n=63),
                dict(slots=(1,), n=257), dict(slots=(2, 3), n=64)):   # the last: slot 2 belongs to group 1
        with pytest.raises(ValueError):
            g.set(0, bad["slots"], bad["n"])
    assert g.members(0) == () and g.seq_prefix.tolist() == [256, 0, 256, 0, 0, 0, 0, 0]
    for bad in (dict(max_prefix=32), dict(max_prefix=100), dict(num_groups=0), dict(group_cap=0), dict(max_batch=0)):
        with pytest.raises(ValueError):
            PrefixGroups(**dict(dict(num_groups=1, group_cap=1, max_batch=1, max_prefix=64, device="cpu"), **bad))


def test_prefix_groups_validate_against_the_page_table():
    t = PageTable(num_pages=16, page_size=64, max_batch=4, pages_per_seq=6, device="cpu")
    t.reserve(0, 200)
    t.fork(0, 1, 200)
    t.reserve(2, 200)
    t.reserve(3, 100)
    g = PrefixGroups(num_groups=2, group_cap=3, max_batch=4, max_prefix=256, device="cpu", page_table=t)
    g.set(0, (0, 1), 192)         # three whole pages in common
    g.set(0, (1, 0), 200)         # .. which cover the 64-key tiles of 200 tokens as well (the kernels round down to 192)
    with pytest.raises(ValueError, match="in common"):
        g.set(1, (2, 3), 64)      # each holds pages of its own
    with pytest.raises(ValueError, match="in common"):
        g.set(0, (0, 1), 256)     # the fourth page is a copy
    assert g.members(0) == (1, 0) and g.prefix(0) == 200


# ------------------------------------------------------------------------------------------------------------------------
# the needle batches are sound, and every mutant of the restatement is seen
# ------------------------------------------------------------------------------------------------------------------------
def _run(sb, chunk, mutant=None, table=None):
    return O.shared(sb.q, sb.k_pool, sb.v_pool, sb.table if table is None else table, sb.lens, sb.bound, sb.members, sb.group_prefix,
                    sb.seq_prefix, sb.max_prefix, chunk, chunk, sb.scale, sb.causal, mutant)


def mutant_applies(sb, mutant: str, chunk: int) -> bool:
    """Whether the construction is bound to see the fault (reasons, not measurements)."""
    s = sb.spec
    if mutant == "noprefix":      # gh 1 seeks the last prefix key of every grouped slot
        return True
    if mutant in ("anchor-64", "anchor+64"):  # the pair (P - 1, P): one half attended twice, or the other never
        return bool(s.get("pair"))
    if mutant == "memberminor":   # another member's (or another head's) q row: group_cap > 1 and G > 1 everywhere
        return True
    if mutant == "leadfirst":     # the first listed slot is inactive: no prefix is written, the members combine NaN
        return any(m[0] >= 0 and sb.lens_spec[m[0]] is None and any(0 <= x < len(sb.lens) and sb.seq_prefix[x] for x in m) for m in sb.members)
    if mutant == "prefixmask":    # row 0 of Sq = 3 would stop two keys before P - 1
        return s["Sq"] > 1
    if mutant == "noclamp":       # the decoy on P - 1 lies behind row 0's causal limit of the short member
        return bool(s.get("decoy")) and chunk == 64
    raise ValueError(mutant)


def test_case_list_covers_the_axes_of_the_issue():
    names = {s["name"] for s in C.CASES}
    assert len(names) == len(C.CASES)
    main = [s for s in C.CASES if s["name"].startswith("main")]
    assert {(s["Dh"], s["Sq"], s["page_size"], s["dtype"]) for s in main} == {(d, q, p, t) for d in (64, 128) for q in (1, 3) for p in (64, 128)
                                                                           for t in (torch.float16, torch.bfloat16)}
    for s in main:
        assert (s["H"], s["Hkv"]) == (8, 2) and C.P == 192
        sb = C.build(s)
        Sq = s["Sq"]
        assert sb.members[0] == [0, 4, 1, 3, -1] and sb.lens_spec[0] is None and sb.lead[0] == 4
        assert [sb.lens_spec[m] for m in (4, 1, 3)] == [C.P + Sq, C.P + 70, C.P + 130]
        assert sb.members[1] == [2, -1, -1, -1, -1] and sb.seq_prefix[5] == 0 and sb.group_prefix[2] == 0 and sb.seq_prefix[6] == 0
        assert sb.table.stride(0) > sb.table.shape[1] and (sb.table_full[:, sb.pps:] == sb.poison).all()
        k = C.P // s["page_size"]   # whole prefix pages: the same ids in every member's row, different ids behind them
        rows = [sb.pages[m] for m in (4, 1, 3)]
        assert all(r[:k] == rows[0][:k] for r in rows) and len({r[k] for r in rows}) == 3 and sb.pages[2][:k] != rows[0][:k]
        pt = sb.poisoned_table()
        assert (pt[1, :k] == sb.poison).all() and (pt[3, :k] == sb.poison).all() and torch.equal(pt[4], sb.table_full[4]) and torch.equal(pt[2], sb.table_full[2])
    full = [C.build(s) for s in C.CASES if s["name"].startswith("full-tile")]
    assert len(full) == 2 and all(sb.cap * sb.Sq * sb.G == 128 and len(sb.lens) == 32 for sb in full)
    short = [C.build(s) for s in C.CASES if s["name"].startswith("short-member")]
    assert len(short) == 2 and all(sb.lens[1] - sb.Sq < sb.group_prefix[0] and not sb.defined(256)[1] and sb.defined(64).all() for sb in short)


@pytest.mark.parametrize("spec", C.CASES, ids=C.case_id)
def test_restatement_returns_the_targets_and_every_mutant_is_seen(spec):
    sb = C.build(spec)
    for chunk in C.CHUNKS:
        ok = sb.defined(chunk)
        out = _run(sb, chunk)
        assert torch.equal(_bits(out[ok]), _bits(sb.target[ok])), chunk
        # where the contract promises attn_kvcache_paged's bits, the restatement agrees with splitkv itself
        ref = O.paged(sb.q, sb.k_pool, sb.v_pool, sb.table, sb.lens, sb.bound, chunk, sb.scale, sb.causal)
        assert torch.equal(_bits(ref[ok]), _bits(sb.target[ok])), chunk
        # no key below a prefix is fetched through a member's own table
        assert torch.equal(_bits(_run(sb, chunk, table=sb.poisoned_table()[:, :sb.pps])[ok]), _bits(sb.target[ok])), chunk
        for mutant in O.MUTANTS:
            if mutant_applies(sb, mutant, chunk):
                bad = _run(sb, chunk, mutant)
                assert not torch.equal(_bits(bad[ok]), _bits(sb.target[ok])), (mutant, chunk)


def test_every_mutant_is_seen_by_some_case():
    for chunk in C.CHUNKS:
        seen = {m: sum(mutant_applies(C.build(s), m, chunk) for s in C.CASES) for m in O.MUTANTS}
        cannot = {"noclamp"} if chunk == 256 else set()   # (the short member is unspecified there)
        assert all(v > 0 for m, v in seen.items() if m not in cannot), (chunk, seen)


def test_ungrouped_restatement_is_splitkv_on_random_data():
    """With no group the contract is attn_kvcache_paged's: the restatement must be `splitkv` bit for bit, fp32 sums and all."""
    g = torch.Generator().manual_seed(5)
    B, Sq, H, Hkv, Dh, ps, pps = 3, 2, 4, 2, 64, 64, 5
    q = torch.randn(B, Sq, H, Dh, generator=g).to(torch.bfloat16)
    k_pool, v_pool = (torch.randn(B * pps + 1, ps, Hkv, Dh, generator=g).to(torch.bfloat16) for _ in range(2))
    table = torch.randperm(B * pps, generator=g).reshape(B, pps).int()
    lens = [300, 70, 0]
    out = O.shared(q, k_pool, v_pool, table, lens, 320, [[-1, -1]], [0], [0, 0, 0], 64, 128, 128)
    ref = O.paged(q, k_pool, v_pool, table, lens, 320, 128)
    assert torch.equal(_bits(out), _bits(ref)) and out[:2].any() and not out[2].any()
