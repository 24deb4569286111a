"""The paged KV cache without a GPU: the four exports, every argument check of the C ABI, the host page allocator, the module's and the shim's
refusals, and the soundness of the paged needle batches of tests/attn_paged_cases.py -- the list tests/test_gpu_attention_paged.py runs
through the kernels -- against the torch restatement of the paged call, of the paged store and each of their mutants."""
import ctypes
import inspect
from types import SimpleNamespace

import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from llm_awq_amd.paged_kv import PagePoolExhausted, PageTable
from tests import attn_paged_cases as P

AWQ_ERR_DTYPE, AWQ_ERR_SHAPE, AWQ_ERR_ALIGN, AWQ_ERR_NULL, AWQ_ERR_WORKSPACE = -3, -4, -5, -6, -7
SYMBOLS = ("awq_rope_kv_store_paged_pos", "awq_rope_kv_store_paged_pos_fp8", "awq_attn_kvcache_paged", "awq_attn_kvcache_paged_kv8")


def test_library_engine_and_ops_export_the_paged_surface():
    L = _capi.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in _capi.SIGNATURES, name
    assert L.awq_abi_version() == 1
    eng = llm_awq_amd.load_engine()

    def params(fn):
        doc = fn.__doc__.splitlines()[0]
        return [p.split(":")[0].strip() for p in doc[doc.index("(") + 1:doc.rindex(")")].split(", ")]
    assert params(eng.attn_kvcache_paged) == ["q", "k_pool", "v_pool", "block_table", "seqlens_k", "max_seqlen_k", "seqlen_offset",
                                              "softmax_scale", "causal"]
    assert params(eng.attn_kvcache_paged_kv8) == ["q", "k_pool", "v_pool", "k_scale", "v_scale", "block_table", "seqlens_k", "max_seqlen_k",
                                                  "seqlen_offset", "softmax_scale", "causal"]
    assert params(eng.rope_kv_store_paged_pos) == ["qkv", "freqs_table", "k_pool", "v_pool", "block_table", "cache_seqlens", "nheads", "nheads_kv"]
    assert params(eng.rope_kv_store_paged_pos_fp8) == ["qkv", "freqs_table", "k_pool", "v_pool", "k_scale", "v_scale", "block_table",
                                                       "cache_seqlens", "nheads", "nheads_kv"]
    assert list(inspect.signature(ops.attn_kvcache_paged).parameters) == ["q", "k_pool", "v_pool", "block_table", "seqlens_k", "max_seqlen_k",
                                                                          "seqlen_offset", "softmax_scale", "causal", "k_scale", "v_scale"]
    assert list(inspect.signature(ops.rope_kv_store_paged).parameters) == ["qkv", "freqs_table", "k_pool", "v_pool", "block_table",
                                                                           "cache_seqlens", "nheads", "nheads_kv", "k_scale", "v_scale"]


# ------------------------------------------------------------------------------------------------------------------------
# argument validation: every code, no GPU call
# ------------------------------------------------------------------------------------------------------------------------
def _p16():
    buf = (ctypes.c_char * 8192)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


ATTN_OK = dict(B=2, Sq=1, off=1, bound=4096, pages=40, ps=256, pps=16, trs=20, H=8, Hkv=2, Dh=128, qbs=1024, qrs=1024, kps=256 * 256, krs=256,
               vps=256 * 256, vrs=256, ksps=256 * 2, ksrs=2, vsps=256 * 2, vsrs=2, scale=0.1, causal=1, dtype=0)


def _attn(p, kv8=False, **kw):
    """The workspace stays NULL unless a test gives one, so even a call that passes every other check launches nothing."""
    a = dict(ATTN_OK, q=p, k=p, v=p, ks=p, vs=p, out=p, bt=p, lens=p, ws=None, wsb=0)
    a.update(kw)
    L = _capi.lib()
    head = (a["bt"], a["B"], a["Sq"], a["lens"], a["off"], a["bound"], a["pages"], a["ps"], a["pps"], a["trs"], a["H"], a["Hkv"], a["Dh"], a["qbs"],
            a["qrs"], a["kps"], a["krs"], a["vps"], a["vrs"])
    tail = (a["scale"], a["causal"], a["dtype"], a["ws"], a["wsb"], None)
    if kv8:
        return L.awq_attn_kvcache_paged_kv8(a["q"], a["k"], a["v"], a["ks"], a["vs"], a["out"], *head, a["ksps"], a["ksrs"], a["vsps"], a["vsrs"],
                                            *tail)
    return L.awq_attn_kvcache_paged(a["q"], a["k"], a["v"], a["out"], *head, *tail)


@pytest.mark.parametrize("kv8", [False, True], ids=["T", "kv8"])
def test_attn_kvcache_paged_argument_validation_returns_codes_without_launch(kv8):
    buf, p = _p16()
    for bad in (dict(ps=0), dict(ps=32), dict(ps=63), dict(ps=96), dict(ps=320 - 1), dict(ps=-64), dict(pages=0), dict(pages=-1), dict(pps=0),
                dict(pps=-2), dict(trs=15), dict(trs=0), dict(bound=4097), dict(pps=15, trs=15), dict(bound=0), dict(off=-1), dict(Dh=96),
                dict(H=6, Hkv=4), dict(B=0), dict(Sq=0), dict(Sq=33), dict(qrs=512), dict(krs=128), dict(vrs=128), dict(qbs=-8), dict(kps=-256),
                dict(vps=-256)):
        assert _attn(p, kv8, **bad) == AWQ_ERR_SHAPE, bad
    assert _attn(p, kv8) == AWQ_ERR_WORKSPACE               # everything else is in order
    assert _attn(p, kv8, ps=64, pps=64, trs=64) == AWQ_ERR_WORKSPACE and _attn(p, kv8, trs=16) == AWQ_ERR_WORKSPACE
    assert _attn(p, kv8, ps=192, pps=22, trs=22) == AWQ_ERR_WORKSPACE   # a multiple of 64 that is no power of two
    assert _attn(p, kv8, pages=1) == AWQ_ERR_WORKSPACE      # one page, named by every entry: the kernel cannot tell
    assert _attn(p, kv8, dtype=2) == AWQ_ERR_DTYPE
    for name in ("q", "k", "v", "out", "bt", "lens") + (("ks", "vs") if kv8 else ()):
        assert _attn(p, kv8, **{name: None}) == AWQ_ERR_NULL, name
    for name in ("q", "k", "v", "out"):
        assert _attn(p, kv8, **{name: p + 2}) == AWQ_ERR_ALIGN, name
    assert _attn(p, kv8, bt=p + 2) == AWQ_ERR_ALIGN and _attn(p, kv8, lens=p + 2) == AWQ_ERR_ALIGN
    assert _attn(p, kv8, bt=p + 4) == AWQ_ERR_WORKSPACE     # four bytes are enough for the table
    if kv8:
        assert _attn(p, kv8, ks=p + 2) == AWQ_ERR_ALIGN and _attn(p, kv8, vs=p + 2) == AWQ_ERR_ALIGN
        assert _attn(p, kv8, ksrs=1) == AWQ_ERR_SHAPE and _attn(p, kv8, vsrs=1) == AWQ_ERR_SHAPE
        assert _attn(p, kv8, ksps=-2) == AWQ_ERR_SHAPE and _attn(p, kv8, vsps=-2) == AWQ_ERR_SHAPE
        for name, val in (("kps", 256 * 256 + 8), ("krs", 264), ("vps", 256 * 256 + 8), ("vrs", 264)):  # strides in codes: multiples of 16
            assert _attn(p, kv8, **{name: val}) == AWQ_ERR_ALIGN, name
    for name, val in (("qbs", 1028), ("qrs", 1028), ("kps", 256 * 256 + 4), ("krs", 260), ("vps", 256 * 256 + 4), ("vrs", 260)):
        assert _attn(p, kv8, **{name: val}) == AWQ_ERR_ALIGN, name
    need = _capi.lib().awq_attn_kvcache_workspace_bytes(2, 8, 2, 128, 1, 4096)  # the dense entry's workspace
    assert need > 0 and _attn(p, kv8, ws=p, wsb=need - 1) == AWQ_ERR_WORKSPACE and _attn(p, kv8, ws=p + 4, wsb=need) == AWQ_ERR_ALIGN


@pytest.mark.parametrize("fp8", [False, True], ids=["T", "fp8"])
def test_store_paged_argument_validation_returns_codes_without_launch(fp8):
    """Every call here is refused: a call that passed would launch, and there is no GPU."""
    buf, p = _p16()
    L = _capi.lib()
    ok = dict(qkv=p, fr=p, q=p, kc=p, vc=p, ks=p, vs=p, bt=p, lens=p, B=2, S=4, H=8, Hkv=2, Dh=128, rot=128, rows=64, pages=9, ps=64, pps=4, trs=6,
              kps=64 * 256, krs=256, vps=64 * 256, vrs=256, ksps=128, ksrs=2, vsps=128, vsrs=2, bs=4 * 1536, rs=1536, dtype=0)

    def call(**kw):
        a = dict(ok, **kw)
        head = (a["bt"], a["lens"], a["B"], a["S"], a["H"], a["Hkv"], a["Dh"], a["rot"], a["rows"], a["pages"], a["ps"], a["pps"], a["trs"],
                a["kps"], a["krs"], a["vps"], a["vrs"])
        tail = (a["bs"], a["rs"], a["dtype"], None)
        if fp8:
            return L.awq_rope_kv_store_paged_pos_fp8(a["qkv"], a["fr"], a["q"], a["kc"], a["vc"], a["ks"], a["vs"], *head, a["ksps"], a["ksrs"],
                                                     a["vsps"], a["vsrs"], *tail)
        return L.awq_rope_kv_store_paged_pos(a["qkv"], a["fr"], a["q"], a["kc"], a["vc"], *head, *tail)
    for bad in (dict(ps=0), dict(ps=32), dict(ps=100), dict(ps=-64), dict(pages=0), dict(pps=0), dict(trs=3), dict(Dh=96), dict(rot=24),
                dict(rot=144), dict(B=0), dict(S=0), dict(H=0), dict(Hkv=0), dict(rows=0), dict(rs=1528), dict(bs=-8), dict(krs=128), dict(vrs=128),
                dict(kps=-256), dict(vps=-256)) + ((dict(ksrs=1), dict(vsrs=1), dict(ksps=-2), dict(vsps=-2)) if fp8 else ()):
        assert call(**bad) == AWQ_ERR_SHAPE, bad
    assert call(dtype=2) == AWQ_ERR_DTYPE
    for name in ("qkv", "fr", "q", "kc", "vc", "bt", "lens") + (("ks", "vs") if fp8 else ()):
        assert call(**{name: None}) == AWQ_ERR_NULL, name
    for name in ("qkv", "fr", "q", "kc", "vc"):
        assert call(**{name: p + 4}) == AWQ_ERR_ALIGN, name
    assert call(bt=p + 2) == AWQ_ERR_ALIGN and call(lens=p + 2) == AWQ_ERR_ALIGN
    if fp8:
        assert call(ks=p + 2) == AWQ_ERR_ALIGN and call(vs=p + 2) == AWQ_ERR_ALIGN
        for name, val in (("kps", 64 * 256 + 8), ("krs", 264), ("vps", 64 * 256 + 8), ("vrs", 264)):
            assert call(**{name: val}) == AWQ_ERR_ALIGN, name
    for name, val in (("kps", 64 * 256 + 4), ("krs", 260), ("vps", 64 * 256 + 4), ("vrs", 260), ("bs", 4 * 1536 + 4), ("rs", 1540)):
        assert call(**{name: val}) == AWQ_ERR_ALIGN, name


def test_ops_refuse_cpu_tensors_and_name_the_shapes():
    q = torch.zeros(2, 1, 8, 128, dtype=torch.float16)
    pool = torch.zeros(4, 64, 2, 128, dtype=torch.float16)
    bt = torch.zeros(2, 4, dtype=torch.int32)
    lens = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.attn_kvcache_paged(q, pool, pool, bt, lens, 256)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.rope_kv_store_paged(torch.zeros(2, 1, 12 * 128, dtype=torch.float16), torch.zeros(64, 128), pool, pool, bt, lens, 8, 2)


# ------------------------------------------------------------------------------------------------------------------------
# PageTable
# ------------------------------------------------------------------------------------------------------------------------
def test_page_table_reserves_releases_and_reuses_pages_in_place():
    t = PageTable(num_pages=6, page_size=64, max_batch=3, pages_per_seq=4, device="cpu")
    ptr = t.table.data_ptr()
    assert t.table.dtype == torch.int32 and tuple(t.table.shape) == (3, 4) and t.free_pages == 6 and not t.table.any()
    assert t.reserve(0, 1) == (0,) and t.reserve(1, 65) == (1, 2) and t.free_pages == 3
    assert t.reserve(0, 64) == () and t.free_pages == 3                 # still covered: nothing new
    assert t.reserve(0, 65) == (3,) and t.table[0].tolist() == [0, 3, 0, 0] and t.table[1].tolist() == [1, 2, 0, 0]
    assert t.pages(0) == (0, 3) and t.pages(2) == ()
    assert t.release(1) == 2 and t.free_pages == 4 and not t.table[1].any()
    got = t.reserve(2, 200)                                              # four pages: the released ones come back first
    assert len(got) == 4 and set(got) == {1, 2, 4, 5} and t.table[2].tolist() == list(got) and t.free_pages == 0
    with pytest.raises(PagePoolExhausted, match=r"1 more pages.*0 of 6 are free"):
        t.reserve(0, 129)
    assert t.table[0].tolist() == [0, 3, 0, 0] and t.free_pages == 0     # a refused reserve changes nothing
    with pytest.raises(ValueError, match="5 pages"):
        t.reserve(1, 257)                                                # more than a table row holds
    assert t.release(2) == 4 and t.release(2) == 0 and t.free_pages == 4
    assert t.reserve(1, 256) and t.free_pages == 0
    held = [p for s in range(3) for p in t.pages(s)]
    assert sorted(held) == list(range(6))                                # no page is held twice
    assert t.table.data_ptr() == ptr                                     # updated in place: a captured graph follows it
    for bad in (dict(page_size=32), dict(page_size=96), dict(num_pages=0), dict(max_batch=0), dict(pages_per_seq=0)):
        with pytest.raises(ValueError):
            PageTable(**dict(dict(num_pages=4, page_size=64, max_batch=1, pages_per_seq=2, device="cpu"), **bad))


def test_page_table_holds_the_ragged_batch_in_a_fraction_of_the_dense_rectangle():
    lens = (131072, 32768, 8192, 2048, 2048, 512, 64)  # README's ragged batch; slot 7 is inactive
    for ps, pages in ((64, 2761), (256, 691), (1024, 174)):
        t = PageTable(num_pages=pages, page_size=ps, max_batch=8, pages_per_seq=131072 // ps, device="cpu")
        for slot, n in enumerate(lens):
            t.reserve(slot, n)
        assert t.free_pages == 0 and pages * ps <= 8 * 131072 // 5     # at most a fifth of the dense rectangle's rows


# ------------------------------------------------------------------------------------------------------------------------
# the module and the shim
# ------------------------------------------------------------------------------------------------------------------------
class _Boom(torch.nn.Module):
    def forward(self, x):
        raise AssertionError("the projection must not run")


def _module(kv_layout, L=128):
    from llm_awq_amd.fused_attn import QuantLlamaAttentionFused

    args = SimpleNamespace(num_attention_heads=8, hidden_size=512, num_key_value_heads=2, rope_theta=10000.0)
    return QuantLlamaAttentionFused(512, 8, L, _Boom(), _Boom(), "cpu", args, max_batch_size=2, kv_layout=kv_layout)


def test_module_refuses_a_block_table_it_cannot_serve_before_any_work():
    x, pos, freqs, bt = torch.zeros(2, 1, 512), torch.zeros(2, dtype=torch.int32), torch.zeros(128, 64), torch.zeros(2, 2, dtype=torch.int32)
    with pytest.raises(ValueError, match="natural"):
        _module("ft")(x, pos, freqs, block_table=bt, page_size=64)
    m = _module("natural")
    with pytest.raises(ValueError, match="start_pos"):
        m(x, 5, freqs, block_table=bt, page_size=64)                    # an int start_pos
    with pytest.raises(ValueError, match="come together"):
        m(x, pos, freqs, block_table=bt)
    with pytest.raises(ValueError, match="come together"):
        m(x, pos, freqs, page_size=64)
    for ps in (32, 96, 256):                                            # not a multiple of 64; does not divide kv_max_seq_len = 128
        with pytest.raises(ValueError, match="page_size"):
            m(x, pos, freqs, block_table=bt, page_size=ps)
    assert not m.cache_k.any() and not m.cache_v.any()
    params = list(inspect.signature(m.forward).parameters)
    assert params[:6] == ["x", "start_pos", "freqs", "mask", "chunk_prefilling", "decode_max_seqlen"] and params[6:] == ["block_table", "page_size"]


def test_flash_attn_with_kvcache_still_refuses_a_block_table_and_points_at_the_paged_op():
    from llm_awq_amd import flash_attn_compat as F

    q = torch.zeros(2, 1, 8, 128, dtype=torch.float16)
    kc = torch.zeros(2, 256, 2, 128, dtype=torch.float16)
    with pytest.raises(NotImplementedError, match="block_table") as e:
        F.flash_attn_with_kvcache(q, kc, kc, cache_seqlens=torch.tensor([5, 9], dtype=torch.int32), causal=True,
                                  block_table=torch.zeros(2, 4, dtype=torch.int32))
    assert "ops.attn_kvcache_paged" in str(e.value)
    with pytest.raises(NotImplementedError, match="softcap") as e:
        F.flash_attn_with_kvcache(q, kc, kc, cache_seqlens=7, softcap=30.0)
    assert "attn_kvcache_paged" not in str(e.value)


# ------------------------------------------------------------------------------------------------------------------------
# the needle batches are sound, and every mutant of the restatement is seen
# ------------------------------------------------------------------------------------------------------------------------
def test_case_list_covers_the_axes_of_the_issue():
    from tests import attn_kvcache_cases as K

    names = {s["name"] for s in P.CASES}
    assert len(names) == len(P.CASES) == 2 * len(K.CASES) + 4
    assert P.PAGE_SIZES == (64, 128) and P.CHUNKS == (64, 256) and P.PAD_COLS > 0
    for ps in P.PAGE_SIZES:
        mine = [s for s in P.CASES if s["page_size"] == ps and not s["share"]]
        assert {(s["Sq"], s["lens"], s["bound"]) for s in mine} == set(K.SHAPES)
        assert sum(s["share"] for s in P.CASES if s["page_size"] == ps) == 2
    pb = P.PagedBatch(next(s for s in P.CASES if s["share"] and s["page_size"] == 64))
    assert pb.pages[0][0] == pb.pages[1][0] and pb.pages[0][1] != pb.pages[1][1]
    assert pb.table_full.stride(0) == pb.pps + P.PAD_COLS and pb.table.stride(0) > pb.table.shape[1]


@pytest.mark.parametrize("spec", P.CASES, ids=P.case_id)
def test_restatement_returns_the_targets_and_every_mutant_is_seen(spec):
    pb = P.PagedBatch(spec)  # (asserts the gather and the NaN of every row that holds no key)
    for chunk in P.CHUNKS:
        out = P.paged(pb, chunk)
        assert torch.equal(out.view(torch.int16), pb.batch.target.view(torch.int16)), chunk
        for mutant in P.MUTANTS:
            if P.mutant_applies(pb, mutant, chunk):
                bad = P.paged(pb, chunk, mutant)
                assert not torch.equal(bad.view(torch.int16), pb.batch.target.view(torch.int16)), (mutant, chunk)


def test_every_mutant_is_seen_by_some_case_of_every_page_size_it_can_show_at():
    for ps in P.PAGE_SIZES:
        for chunk in P.CHUNKS:
            seen = {m: 0 for m in P.MUTANTS}
            for spec in P.CASES:
                if spec["page_size"] == ps and spec["dtype"] == torch.float16:
                    pb = P.PagedBatch(spec)
                    for m in P.MUTANTS:
                        seen[m] += P.mutant_applies(pb, m, chunk)
            cannot = set()
            if ps == 64:
                cannot.add("slot64")     # a 64-row page has no row 64
            if chunk <= ps:
                cannot.add("firstpage")  # a split holds one page
            assert all(v > 0 for m, v in seen.items() if m not in cannot), (ps, chunk, seen)
            assert all(seen[m] == 0 for m in cannot), (ps, chunk, seen)


STORE_POS = {1: (0, 63, 64, 130, -1, 10 ** 6), 5: (62, 126, 0, 60, -1, 10 ** 6)}


@pytest.mark.parametrize("S_", [1, 5])
@pytest.mark.parametrize("ps", P.PAGE_SIZES)
def test_store_restatement_and_its_mutant(S_, ps):
    pb = P.PagedBatch(next(s for s in P.CASES if s["page_size"] == ps and s["Sq"] == 1 and s["bound"] == 257 and not s["share"]))
    B = pb.table.shape[0]
    pos = STORE_POS[S_]
    assert len(pos) == B
    g = torch.Generator().manual_seed(S_ + ps)
    # every sequence owns all the pages of its row here: a table of its own over a fresh pool
    pb.num_pages = B * pb.pps + 1
    pb.table_full = torch.full((B, pb.pps + P.PAD_COLS), B * pb.pps, dtype=torch.int32)
    pb.table_full[:, :pb.pps] = torch.randperm(B * pb.pps, generator=g).reshape(B, pb.pps).int()
    pb.table = pb.table_full[:, :pb.pps]
    Hkv, Dh = 2, 64
    k0 = torch.zeros(pb.num_pages, ps, Hkv, Dh)
    new_k, new_v = torch.randn(B, S_, Hkv, Dh, generator=g), torch.randn(B, S_, Hkv, Dh, generator=g)
    # the dense store: cache[b, pos + s] = new[b, s], then scattered page by page
    dense_k, dense_v = torch.zeros(B, pb.pps * ps, Hkv, Dh), torch.zeros(B, pb.pps * ps, Hkv, Dh)
    for b, p0 in enumerate(pos):
        if 0 <= p0 and p0 + S_ <= pb.pps * ps:
            dense_k[b, p0:p0 + S_], dense_v[b, p0:p0 + S_] = new_k[b], new_v[b]
    want_k, want_v = k0.clone(), k0.clone()
    want_k[pb.table.long()] = dense_k.reshape(B, pb.pps, ps, Hkv, Dh)
    want_v[pb.table.long()] = dense_v.reshape(B, pb.pps, ps, Hkv, Dh)
    got_k, got_v = P.stored(pb, k0, k0, new_k, new_v, pos)
    assert torch.equal(got_k, want_k) and torch.equal(got_v, want_v) and got_k.any()
    assert not got_k[B * pb.pps].any()  # the poison page is nobody's
    crosses = P.store_mutant_applies(pb, pos, S_, "pos-page")
    assert crosses == (S_ == 5)  # 62 .. 66 crosses at both page sizes, 126 .. 130 too
    bad_k, _ = P.stored(pb, k0, k0, new_k, new_v, pos, mutant="pos-page")
    assert torch.equal(bad_k, want_k) != crosses
