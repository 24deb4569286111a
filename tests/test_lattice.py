"""CPU side of the integer-lattice parity (tests/helpers.py make_lattice_case / lattice_oracle; the GPU sweep is tests/test_gpu_lattice.py):

* the invariant holds for every shape the GPU sweep uses (sum |x||w| < 2^24 * 2^e0 bounds every partial sum; fp16 outputs stay finite);
* the lattice weights (q - z) * s are the pinned oracle's dequantised weights bit for bit, and the oracle's forward / fp32 partial equal
  `lattice_oracle` bit for bit -- with and without bias, bf16 and fp16, W4 and W3: the exact answer IS the reference's answer;
* the sz_half side buffer of the lattice is exact (the f16-mantissa dequant path runs on the GPU);
* the lattice really exercises the rounding tie: at least 0.1 % of the bf16 outputs are exact RNE ties at every K of the sweep."""
import numpy as np
import pytest
import torch

from oracle import awq_oracle as O
from tests.helpers import (assert_lattice_equal, lattice_bias, lattice_oracle, lattice_radius, lattice_weight_f64, make_lattice_case,
                           rne_ties)
from tests.test_gpu_lattice import EDGE, LAYERS, MOE, PAIRS

DTYPES = [torch.bfloat16, torch.float16]


def _all_gpu_shapes():
    out = set()
    for (_name, K, N, bits) in LAYERS + EDGE:
        out.add((K, N, bits))
    for (_name, K, F, bits) in PAIRS:
        out.add((K, 2 * F, bits))
    for (K, N) in MOE:
        out.add((K, N, 4))
    return sorted(out)


@pytest.mark.parametrize("dtype", DTYPES)
def test_invariant_holds_for_every_gpu_shape(dtype):
    for (K, N, bits) in _all_gpu_shapes():
        R = lattice_radius(K, bits, -9, dtype)
        assert R >= 1, (K, N, bits)
        bound = K * R * (2 ** bits - 1) * 7 * 2
        assert bound < 2 ** 24, (K, N, bits, R)
        if dtype == torch.float16:
            assert bound * 2.0 ** -9 < 65504, (K, N, R)
        # (the helper asserts the same for the case it builds: a small N of this K)
        make_lattice_case(16, K, dtype, seed=K, M=2, bits=bits)


def test_radius_follows_k():
    assert lattice_radius(4096) >= 8 and lattice_radius(14336) >= 4 and lattice_radius(28672) >= 2
    with pytest.raises(AssertionError):
        make_lattice_case(16, 4096, torch.bfloat16, M=1, R=lattice_radius(4096) + 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bits", [4, 3])
def test_lattice_weights_are_the_oracle_dequant(dtype, bits):
    c = make_lattice_case(64, 384, dtype, seed=3 + bits, M=4, bits=bits)
    W = O.dequant_weight(c["q"], c["scales"], c["scaled_zeros"], 128)
    assert torch.equal(W.double(), lattice_weight_f64(c)), "(q - z) * s must be the oracle's T(q * s + sz) bit for bit"
    if bits == 4:
        qw = torch.from_numpy(O.pack_v2(c["q"]))
        assert (O.unpack_v2(qw.numpy()) == c["q"]).all()
    else:
        assert (O.unpack_w3(O.pack_w3(c["q"])) == c["q"]).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bits", [4, 3])
@pytest.mark.parametrize("N,K", [(48, 128), (64, 1024), (32, 4096)])
def test_oracle_forward_and_partial_equal_the_lattice_oracle(dtype, bits, N, K):
    c = make_lattice_case(N, K, dtype, seed=N * 7 + K + bits, M=9, bits=bits)
    x = c["x"]
    y, y32, _ = lattice_oracle(x, c)
    got = O.wqlinear_forward(x, None, c["scales"], c["scaled_zeros"], None, 128, q_int=c["q"])
    assert_lattice_equal(got, y, "oracle forward")
    b = lattice_bias(c, seed=N + K)
    yb, _, _ = lattice_oracle(x, c, bias=b)
    got_b = O.wqlinear_forward(x, None, c["scales"], c["scaled_zeros"], b, 128, q_int=c["q"])
    assert_lattice_equal(got_b, yb, "oracle forward + bias")
    p = O.wqlinear_partial_f32(x, None, c["scales"], c["scaled_zeros"], 128, q_int=c["q"])
    assert_lattice_equal(p, y32, "oracle fp32 partial")
    # (the reference's bias order matters on the lattice: one rounding of acc + b is another answer on some outputs)
    if K >= 1024:
        once = (y32 + b.float()).to(dtype)
        assert not torch.equal(once.view(torch.int16), yb.view(torch.int16)), "the lattice bias must separate T(acc + b) from T(T(acc) + b)"


@pytest.mark.parametrize("dtype", DTYPES)
def test_sz_half_of_the_lattice_is_exact(dtype):
    for (N, K) in ((16, 128), (272, 1024), (64, 4096)):
        c = make_lattice_case(N, K, dtype, seed=N + K)
        _packed, exact = O.pack_sz_half(c["scales"], c["scaled_zeros"], K)
        assert exact, (N, K, dtype)


@pytest.mark.parametrize("K", sorted({k for (k, _n, _b) in _all_gpu_shapes()}))
def test_ties_are_exercised_in_bf16(K):
    c = make_lattice_case(256, K, torch.bfloat16, seed=K, M=16)
    y, y32, ties = lattice_oracle(c["x"], c)
    assert ties >= 0.001 * y.numel(), f"K={K}: {ties} ties of {y.numel()} outputs"


def test_tie_detector():
    v = torch.tensor([257.0, 256.0, 258.0, 259.0, -257.0, 0.0, 513.0, 515.0, 1.0 + 2 ** -8, 3 * 2 ** -9])
    # bf16: 8 significant bits -- 257 and 259 lie halfway between neighbours spaced 2 apart, 513 / 515 between neighbours spaced 4 apart are not
    assert rne_ties(v, torch.bfloat16).tolist() == [True, False, False, True, True, False, False, False, True, False]
    assert rne_ties(torch.tensor([2049.0, 2048.0, 1.0 + 2 ** -11]), torch.float16).tolist() == [True, False, True]
