"""numpy restatement of the token log-probability contract (include/awq_cdna4.h: awq_lm_head_logprobs, awq_token_logprobs; DESIGN.md "Token
log-probabilities") in float64, the builders of the test cases, the derived bounds and one mutant per fault the GPU tests must see.

The contract, per row t of x (T = bf16 or fp16); steps 1 - 2 are tests/lm_head_oracle.py's (imported, not restated):
  0. targets[t] outside [0, V): the row is ignored -- its outputs keep what they held; its x, NaN included, changes no other row.
  1. z[t, v] = sum_k f32(xn[t, k]) f32(W[v, k]) (+ f32(bias[v])) in fp32; with round_logits, z is rounded once to T, nearest-even.
  2. lse[t] = log sum_v exp(z[t, v]);  argmax[t] = the lowest v among the maxima of z[t, :].
  3. target_logit[t] = z[t, targets[t]];  logprob[t] = target_logit[t] - lse[t], one fp32 subtraction.

The bound on lse (derived, not measured).  Write b_v for the logit bound of lm_head_oracle, (K + 1) 2^-24 (sum_k |xn w| + |bias|), which is ZERO on
the integer lattice; off the lattice with round_logits the reference is the lse of the UNROUNDED float64 logits and ulp_T(|z| + b) / 2 is added
to b_v.  u = 2^-24.
  a. lse is 1-Lipschitz in the sup norm: the logit errors move it by at most max_v b_v.
  b. The kernels sum e_v = exp(z_v - m) over a tree whose leaves are the V columns; m is the maximum of the columns summed so far, and where two
     partial sums with maxima m1 >= m2 meet, the second is multiplied by exp(m2 - m1).  A leaf therefore reaches the root as a product of at most
     LEVELS exponentials whose arguments d_1 + ... + d_L = d_v = max - z_v are all >= 0.  Each exponential exp(d) is computed as
     v_exp_f32((a - b) * log2e): the subtraction is rounded (|d| u), the product is rounded (|d| u in natural units) and log2e itself is an fp32
     constant (|d| u): 3 |d| u in the argument, which is the relative error of the result; summed over the levels that is 3 d_v u, whatever the
     split.  v_exp_f32 is taken at 1 ulp (2^-23 relative: the convention of tests/tail_oracle.py), and each level's product is rounded once (u):
     LEVELS (2^-23 + u) more.  A result below the smallest normal number may be flushed: 2^-126 absolute per leaf, against a sum that is >= 1.
     Weighting every leaf by its share p_v = e_v / sum e of the sum gives the relative error of S from the terms,
         sum_v p_v (3 d_v u + LEVELS (2^-23 + u)) + V 2^-126,
     and a sum of n positive fp32 terms in any order adds a relative (n - 1) u, n = V + the number of vocabulary tiles (the partial sums count as
     terms: generous, the tree has V - 1 additions).  These are first-order statements; the product of (1 + delta) factors is covered by a factor
     1.01 (the total is far below 1e-2).  d log S = dS / S: the relative error of S is the absolute error of log S.
  c. log S = v_log_f32(S) * ln2: 1 ulp of the hardware logarithm (2^-23 |log2 S|, and not less than 2^-23 ln2: one ulp at 1, where its relative
     accuracy next to S = 1 is not relied upon), one rounding of the product and ln2 as an fp32 constant (2 u |log S|); M + log S is rounded once
     (u |lse|).
  d. logprob = target_logit - lse: b_target + the lse bound + one rounding, u |logprob|.
LEVELS is 4 for the fused pair (the lane's 16 registers, the lane pair, the two waves that split the tile, the combine) and 1 for awq_token_logprobs
(two passes: every term is exp(z - M) with the final M).

On the lattice the logit error is zero: target_logit must EQUAL the float64 value (its nearest-even rounding under round_logits) and argmax is exact.
"""
import numpy as np
import torch

from tests import lm_head_oracle as H

U = 2.0 ** -24
LEVELS_FUSED, LEVELS_ROWS = 4, 1
IGNORED = (-1, -100)        # and V itself: the first value past the table
K_VALUES = (8, 40, 72, 136, 1032)

MUTANTS = {
    "v_pad_zero": "padding columns of the last tile enter the sum as exp(0)",
    "k_tail": "K tail dropped",
    "max_init_zero": "running max starts at 0: wrong when a row's logits are all below about -100",
    "no_rescale": "tiles summed without exp(m_t - M)",
    "bias_not_in_lse": "bias missing from the lse",
    "target_tile_off_by_one": "target in the first / last column of a tile read from the neighbouring column",
    "round_skipped": "round_logits not applied",
    "argmax_highest_tie": "ties broken toward the highest index",
    "ignored_written": "outputs of an ignored row overwritten",
    "nan_leak": "an ignored row's NaN reaches another row",
    "row_prev": "row t uses row t - 1's data",
    "ldx_as_k": "the row stride taken as K",
}


def lattice_shapes(rt, vt):
    """about twenty (T, V, K): every T in {1, 2, rt - 1, rt, rt + 1, 2 rt + 5}, V in {1, 17, vt - 1, vt, vt + 1, 2 vt + 17} and K in K_VALUES at least twice"""
    ts, vs = [1, 2, rt - 1, rt, rt + 1, 2 * rt + 5], [1, 17, vt - 1, vt, vt + 1, 2 * vt + 17]
    shapes = []
    for i in range(20):
        shapes.append((ts[i % 6], vs[(i + i // 6) % 6], K_VALUES[i % 5]))
    return shapes


def logsumexp(z):
    m = z.max(-1, keepdims=True)
    return (m + np.log(np.exp(z - m).sum(-1, keepdims=True)))[..., 0]


def from_logits(z, targets=None, init=None, mutant=None, vt=128, z_lse=None):
    """steps 0, 2, 3 on float64 logits z [T, V].  z_lse: the logits the lse is taken of (the bias-less ones for a mutant).  init: dict of what the
    outputs held.  Returns dict(logprob, lse, target_logit, argmax) of float64 / int64 [T]."""
    T, V = z.shape
    zl = z if z_lse is None else z_lse
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if mutant == "v_pad_zero":
            zl = np.concatenate([zl, np.zeros((T, (-V) % vt))], axis=1)
        if mutant == "max_init_zero":
            m = np.maximum(zl.max(-1), 0.0)
            s = np.exp(zl - m[:, None]).astype(np.float32).astype(np.float64).sum(-1)   # terms below fp32's range are gone
            lse = m + np.log(s)
        elif mutant == "no_rescale":
            pad = np.concatenate([zl, np.full((T, (-zl.shape[1]) % vt), -np.inf)], axis=1).reshape(T, -1, vt)
            mt = pad.max(-1)
            st = np.exp(pad - mt[..., None]).sum(-1)
            lse = mt.max(-1) + np.log(st.sum(-1))
        else:
            lse = logsumexp(zl)
    if mutant == "argmax_highest_tie":
        am = V - 1 - np.argmax(z[:, ::-1], axis=-1)
    else:
        am = np.argmax(z, axis=-1)                       # numpy returns the first of equal maxima
    out = {"lse": lse, "argmax": am.astype(np.int64)}
    active = np.ones(T, bool)
    if targets is not None:
        tg = np.asarray(targets).astype(np.int64)
        active = (tg >= 0) & (tg < V)
        col = np.where(active, tg, 0)
        if mutant == "target_tile_off_by_one":
            col = np.where(col % vt == 0, np.maximum(col - 1, 0), np.where(col % vt == vt - 1, np.minimum(col + 1, V - 1), col))
        tl = z[np.arange(T), col]
        out["target_logit"] = tl
        out["logprob"] = tl - lse
    if mutant == "ignored_written":
        active = np.ones(T, bool)
    for name in out:
        held = np.zeros(T) if init is None or name not in init else np.asarray(init[name], dtype=np.float64)
        out[name] = np.where(active, out[name], held)
    out["active"] = active
    return out


def reference(x_store, ldx, T, w, bias=None, targets=None, round_logits=False, dtype_name="bf16", init=None, mutant=None, vt=128, lattice=True):
    """the whole contract in float64 from the storage of x (row t at t * ldx), W [V, K] and bias [V] as float64 arrays of T values.  Off the lattice
    (lattice=False) the logits are left unrounded under round_logits: the bound then carries ulp_T / 2.  Returns from_logits' dict, plus z and absdot."""
    V = w.shape[0]
    hm = mutant if mutant in ("k_tail", "row_prev", "ldx_as_k", "nan_leak") else None
    seq = None
    if targets is not None:
        tg = np.asarray(targets).astype(np.int64)
        seq = np.where((tg >= 0) & (tg < V), 1, -1)
    rounded = round_logits and lattice and mutant != "round_skipped"
    # (lm_head_oracle.reference writes only active rows; every row is wanted here, the ignored ones are dropped by from_logits)
    z, absdot = H.reference(x_store, ldx, T, w, bias, out="T" if rounded else "f32", dtype_name=dtype_name, mutant=hm,
                            seqlens=seq if hm == "nan_leak" else None)
    if hm == "nan_leak":      # lm_head_oracle leaves the ignored rows at zero; the poisoned neighbours are what matters
        z = np.where((seq < 0)[:, None], np.nan, z)
    z_lse = None
    if mutant == "bias_not_in_lse" and bias is not None:
        z_lse = H.reference(x_store, ldx, T, w, None, out="T" if rounded else "f32", dtype_name=dtype_name)[0]
    with np.errstate(invalid="ignore"):
        res = from_logits(z, targets, init, mutant, vt, z_lse)
    res["z"], res["absdot"] = z, absdot
    return res


def bounds(z, targets=None, logit_bound=0.0, n_tiles=1, levels=LEVELS_FUSED):
    """the docstring's bounds for rows of float64 logits z [T, V]; logit_bound: 0 (lattice), or b [T, V] (with the ulp_T / 2 already in it where it
    applies).  Returns dict(lse, logprob, target_logit) of [T] arrays."""
    T, V = z.shape
    b = np.broadcast_to(np.asarray(logit_bound, dtype=np.float64), z.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        m = z.max(-1, keepdims=True)
        d = m - z
        e = np.exp(-d)
        S = e.sum(-1)
        p = e / S[:, None]
        rel_terms = (p * (3.0 * d * U + levels * (2.0 ** -23 + U))).sum(-1) + V * 2.0 ** -126
        rel_S = 1.01 * (rel_terms + (V + n_tiles - 1) * U)
        logS = np.log(S)
        lse = m[:, 0] + logS
        log_err = np.maximum(np.abs(logS) / np.log(2.0), np.log(2.0)) * 2.0 ** -23 + 2 * U * np.abs(logS)
        out = {"lse": b.max(-1) + rel_S + log_err + U * np.abs(lse)}
        if targets is not None:
            tg = np.asarray(targets).astype(np.int64)
            col = np.where((tg >= 0) & (tg < V), tg, 0)
            out["target_logit"] = b[np.arange(T), col]
            out["logprob"] = out["target_logit"] + out["lse"] + U * (np.abs(z[np.arange(T), col] - lse) + out["target_logit"] + out["lse"])
    return out


def mismatches(got, want, bnd, logit_bound=None):
    """THE check of the GPU tests (and of the proof that the mutants are seen): every element of every output named in `got`.  An ignored row must
    hold exactly what `want` holds (what the output held before); argmax is exact; lse, logprob and target_logit lie within bnd[name] (zero for
    target_logit on the lattice: equality).  A NaN where a number is due is a mismatch.  Off the lattice (logit_bound b [T, V] given, want["z"]
    the float64 logits) two logits closer than their bounds have no order the arithmetic must respect: an argmax j is then also accepted where
    z[j] + b[j] >= z[best] - b[best].  Returns the list of (name, row)."""
    bad = []
    act = want["active"]
    for name in ("logprob", "lse", "target_logit", "argmax"):
        if name not in got:
            continue
        g, w = np.asarray(got[name], dtype=np.float64), np.asarray(want[name], dtype=np.float64)
        tol = np.zeros_like(w) if name == "argmax" else np.where(act, np.nan_to_num(np.asarray(bnd[name], dtype=np.float64), nan=0.0), 0.0)
        with np.errstate(invalid="ignore"):
            ok = np.abs(g - w) <= tol
        ok |= (g == w)                                    # (covers equal infinities)
        if name == "argmax" and logit_bound is not None:
            z, b, rows = want["z"], np.broadcast_to(logit_bound, want["z"].shape), np.arange(len(w))
            j, best = np.clip(g.astype(np.int64), 0, z.shape[1] - 1), np.clip(w.astype(np.int64), 0, z.shape[1] - 1)
            ok |= act & (j == g) & (z[rows, j] + b[rows, j] >= z[rows, best] - b[rows, best])
        bad += [(name, int(t)) for t in np.nonzero(~ok)[0]]
    return bad


def general_logit_bound(res, K, dtype_name, round_logits):
    """b_v for inputs off the lattice: lm_head_oracle.bound, which adds ulp_T / 2 for a T-rounded value"""
    return H.bound(res["absdot"], K, out="T" if round_logits else "f32", dtype_name=dtype_name, y=res["z"])


# ---- builders ----

def edge_targets(T, V, vt, ignored=()):
    """targets that walk column 0, V - 1 and the first and last column of every tile edge that exists; rows named in `ignored` get -1 / -100 / V in turn"""
    cands = sorted({c for c in (0, V - 1, vt - 1, vt, 2 * vt - 1, 2 * vt, V // 2, 1) if 0 <= c < V})
    tg = np.array([cands[t % len(cands)] for t in range(T)], dtype=np.int32)
    for i, t in enumerate(ignored):
        tg[t] = (IGNORED + (V,))[i % 3]
    return tg


def build_lattice(T, V, K, dtype_name, with_bias, vt, seed=0):
    """lm_head_oracle.build_lattice (x as the last token of a [T, 3, K] tensor whose other tokens are NaN, two columns of row 0 on ties of T), plus
    one column that repeats the weights of row 0's best column, so that the maximum is TIED between two indices; targets on the tile edges."""
    c = H.build_lattice(T, V, K, dtype_name, with_bias, seed)
    w, bias = c["w"].clone(), None if c["bias"] is None else c["bias"].clone()
    best = int(np.argmax(c["y_f32"][0]))
    twin = None
    if V >= 4:
        twin = V - 1 if best != V - 1 else V // 2
        w[twin] = w[best]
        if bias is not None:
            bias[twin] = bias[best]
    case = dict(T=T, V=V, K=K, dtype_name=dtype_name, x3=c["x3"], w=w, bias=bias, ldx=c["ldx"], x_store=c["x_store"], tie=(best, twin),
                targets=edge_targets(T, V, vt), vt=vt, ties_T=c["ties"])
    return case


def case_reference(case, round_logits=False, targets="own", init=None, mutant=None, x_store=None):
    tg = case["targets"] if isinstance(targets, str) else targets
    return reference(case["x_store"] if x_store is None else x_store, case["ldx"], case["T"], H.f64(case["w"]),
                     None if case["bias"] is None else H.f64(case["bias"]), tg, round_logits, case["dtype_name"], init, mutant, case["vt"])


def build_extreme(kind, dtype_name, vt, seed=0):
    """exact (lattice) rows at the ends of the range, T = 3, V = vt + 17 (two tiles, the last one partial), K = 8:
       "all_low"  every logit <= -3e4, through a bias of -31744 on every column
       "spike"    one column of the second tile 200 and more above the rest (bias 256 there; the others stay within +-4)
       "equal"    every logit equal (all rows of W alike): lse = z + log V, argmax 0"""
    rng = np.random.default_rng(seed + {"all_low": 1, "spike": 2, "equal": 3}[kind])
    T, V, K = 3, vt + 17, 8
    r = H.R if kind == "all_low" else 16
    xi = rng.integers(-r, r + 1, size=(T, K)).astype(np.float64)
    wi = rng.integers(-r, r + 1, size=(V, K)).astype(np.float64)
    bias = np.zeros(V)
    if kind == "all_low":
        bias[:] = -31744.0
    elif kind == "spike":
        bias[vt + 3] = 256.0
    else:
        wi[:] = wi[0]
    Tt = H.DTYPES[dtype_name]
    x3 = torch.full((T, 3, K), float("nan"), dtype=Tt)
    x3[:, 2, :] = torch.from_numpy(xi * 2.0 ** H.X_EXP).to(Tt)
    w, bt = torch.from_numpy(wi * 2.0 ** H.W_EXP).to(Tt), torch.from_numpy(bias).to(Tt)
    assert np.array_equal(H.f64(bt), bias) and np.array_equal(H.f64(w), wi * 2.0 ** H.W_EXP)
    assert (np.abs(xi) @ np.abs(wi).T + np.abs(bias) * 2.0 ** -(H.X_EXP + H.W_EXP)).max() < 2 ** 24     # exact in fp32 in any order
    case = dict(T=T, V=V, K=K, dtype_name=dtype_name, x3=x3, w=w, bias=bt, ldx=3 * K, x_store=H.f64(x3).reshape(-1)[2 * K:], vt=vt,
                targets=np.array([0, vt + 3, V - 1], dtype=np.int32), kind=kind)
    return case


def ignored_patterns(T, V):
    """targets with -1 / -100 / V at the first, a middle and the last row (all three at once), and the rows they name"""
    rows = sorted({0, T // 2, T - 1})
    return rows


# ---- entry.py:304-326 restated literally, in torch float64 (the reference of evaluate.perplexity) ----

def entry_py_perplexity(logits_fn, testenc, seqlen):
    """logits_fn(batch [1, seqlen]) -> lm_logits [1, seqlen, V] (any float dtype); testenc [1, N] int64"""
    nsamples = testenc.numel() // seqlen
    nlls = []
    for i in range(nsamples):
        batch = testenc[:, (i * seqlen):((i + 1) * seqlen)]
        lm_logits = logits_fn(batch)
        shift_logits = lm_logits[:, :-1, :].contiguous().double()
        shift_labels = testenc[:, (i * seqlen):((i + 1) * seqlen)][:, 1:]
        loss_fct = torch.nn.CrossEntropyLoss()
        loss = loss_fct(shift_logits.view(-1, shift_logits.size(-1)), shift_labels.reshape(-1))
        neg_log_likelihood = loss.double() * seqlen
        nlls.append(neg_log_likelihood)
    return torch.exp(torch.stack(nlls).sum() / (nsamples * seqlen)).item()
