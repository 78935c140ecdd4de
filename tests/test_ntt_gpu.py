"""FR NTT on the device (include/hrx.h hrx_fr_ntt_prepare_device / hrx_fr_ntt_device; csrc/hrx_kernel_ntt.hip) against the host twin, every limb, every buffer
between poisoned guards:
  sizes                every k from 1 to two past the plan's largest one-pass k (every packing factor, the whole-LDS tile, the first multi-pass sizes and a
                       one-bit pass), then every k to 20 — the smallest and the largest of every further pass count, and the sizes between those — one
                       column, forward with a short input and, shifted, inverse in place: every width of a last strided pass
  three passes         the smallest such k: 3 columns with in_pitch != out_pitch and n_in = 2^k - 1, the in-place pair swap of 2 columns with n_in = 2^(k-2),
                       inverse canonical at a wider out_pitch
  the largest sizes    k = 21 .. 24, no host transform of that size: the transform of 2^20 entries coset by coset against 2^(k-20) transforms of size 2^20,
                       a dense column forward and back in place, Python integers at about 40 outputs around every pass border
  columns              1, cols_per_group - 1, cols_per_group, cols_per_group + 1, 5 at a packed and an unpacked k
  argument forms       both directions and limb forms, with and without a shift, n_in in {1, 2^k - 1, 2^(k-2), 2^k} with the unread input poisoned on
                       the device, in place and out of place, in_pitch != out_pitch
  round trips, workspaces of two sizes in turn, one workspace on two streams
  the chain            regex1's A', S', Z columns written at pitch 4096 by the device stages, to coefficients in place (Horner in Python integers), then to
                       the extended coset at k = 14
  contract             capture and replay as a fresh context's first calls, a side stream, two contexts in turn, every refusal with nothing written"""
import contextlib
import gc

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import halo2_regex_amd as hra
import ntt_ref as nr
from compress_ref import R, cell_limbs
from test_compress_gpu import on_device
from test_lookup_gpu import batch
from test_match_cpu import CFG_1, CFG_23, _cfg
from test_permute_gpu import guarded, intact, POISON64
from test_product_cpu import challenges
from test_verify_gpu import defs_of_files

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

_HOST = _cfg(CFG_1, 64)                                                                 # host-only: the plan and the host twin
plan = lambda k: _HOST.fr_ntt_plan(1, k)
P = max(k for k in range(1, 25) if plan(k)["n_passes"] == 1)                            # the largest one-pass k
PACKED = max(k for k in range(1, P + 1) if plan(k)["cols_per_group"] > 1)               # ... and the largest k whose columns share a workgroup


def further_pass_sizes():
    """for every pass count the sizes above P + 2 have below k = 20: its smallest and its largest k"""
    by = {}
    for k in range(P + 3, 21):
        by.setdefault(plan(k)["n_passes"], []).append(k)
    return sorted({ks[0] for ks in by.values()} | {ks[-1] for ks in by.values()})


_CFG, _WS = [], {}


@pytest.fixture(scope="module", autouse=True)
def release_the_shared_context():
    """the module's device context and workspaces go with the module: a device's placement arenas live as long as any context on it does, and later
    modules count on starting without one"""
    yield
    _WS.clear()
    _BIG.clear()
    _CFG.clear()
    gc.collect()


def dev_cfg():
    if not _CFG:
        _CFG.append(hra.RegexVerifyConfig.configure(64, defs_of_files(CFG_1), device=0))
    return _CFG[0]


def workspace(k):
    if k not in _WS:
        raw, ws = guarded(dev_cfg().fr_ntt_workspace_bytes(k) // 8, torch.int64)
        dev_cfg().fr_ntt_prepare(k, workspace=ws.view(torch.int8))
        torch.cuda.synchronize()
        assert intact(raw, ws.numel(), torch.int64)
        _WS[k] = (raw, ws.view(torch.int8), ws.clone())
    return _WS[k][1]


def workspaces_unchanged():
    return all(intact(raw, keep.numel(), torch.int64) and torch.equal(ws.view(torch.int64), keep) for raw, ws, keep in _WS.values())


def columns(n_cols, n_in, pitch, seed, canonical):
    """uint64 cells [n_cols][pitch][4]: seeded elements (0, 1, r - 1 among them) in [0, n_in), poison from there on"""
    rng = np.random.default_rng(seed)
    cells = np.full((n_cols, pitch, 4), POISON64, np.uint64)
    raw = rng.integers(0, 1 << 62, (n_cols, n_in, 4), dtype=np.uint64)                  # elements below 2^252 < r: fully reduced in either limb form
    raw[:, :, 3] >>= 2
    cells[:, :n_in] = raw
    for c in range(n_cols):
        for i, v in enumerate((0, 1, R - 1)[:n_in]):
            cells[c, (i * 7 + c) % n_in] = cell_limbs(v, canonical)
    return cells


def shift_of(g, canonical):
    return None if g is None else np.array(cell_limbs(g, canonical), np.uint64)


def same_as_host(k, n_cols, n_in=None, inverse=False, canonical=False, g=None, in_place=False, out_pitch=None, in_pitch=None, seed=1, cfg=None, stream=None, ws=None,
                 cells=None, shift=None):
    """one device call between guards against the host twin on the same cells; returns the output cells [n_cols][2^k][4]
    (cells: the caller's [n_cols][in_pitch][4] in place of seeded ones; shift: the shift's limbs as they are, reduced or not, in place of g's)"""
    cfg = cfg or dev_cfg()
    n = 1 << k
    n_in = n if n_in is None else n_in
    out_pitch = out_pitch or max(n, 4)
    in_pitch = out_pitch if in_place else (in_pitch or (n_in + 3) & ~3)
    cells = columns(n_cols, n_in, in_pitch, seed, canonical) if cells is None else cells
    assert cells.shape == (n_cols, in_pitch, 4) and cells.dtype == np.uint64
    shift = shift_of(g, canonical) if shift is None else shift
    want = _HOST.fr_ntt_host(cells, k, inverse=inverse, n_in=n_in, shift=shift, canonical=canonical)
    raw_in, d_in = guarded(cells.size, torch.int64)
    d_in = d_in.view(n_cols, in_pitch, 4)
    d_in.copy_(on_device(cells))
    if in_place:
        raw_out, d_out = raw_in, d_in
    else:
        raw_out, d_out = guarded(n_cols * out_pitch * 4, torch.int64)
        d_out = d_out.view(n_cols, out_pitch, 4)
    res = cfg.fr_ntt(d_in, k, workspace=ws if ws is not None else workspace(k), out=d_out, inverse=inverse, n_in=n_in,
                     shift=None if shift is None else on_device(shift), canonical=canonical, stream=stream)
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    assert res.data_ptr() == d_out.data_ptr()
    got = d_out.cpu().numpy().view(np.uint64)
    what = (k, n_cols, n_in, inverse, canonical, g, in_place)
    assert np.array_equal(got[:, :n], want[:, :n]), what
    assert (got[:, n:] == POISON64).all(), ("entries above 2^k", what)
    assert intact(raw_out, d_out.numel(), torch.int64) and intact(raw_in, d_in.numel(), torch.int64), what
    if not in_place:
        assert np.array_equal(d_in.cpu().numpy().view(np.uint64), cells), ("the input", what)
    return got[:, :n]


G = 0x1f3c5a7e9b2d4f6081a3c5e7092b4d6f8fa1c3e507294b6d8fb1d3f517395b7d % R


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(1, P + 3))
def test_every_size_up_to_two_past_the_one_pass_limit(k):
    cpg = plan(k)["cols_per_group"]
    n_cols = cpg + 1 if cpg > 1 else 2
    same_as_host(k, n_cols, g=G, seed=k)
    same_as_host(k, n_cols, inverse=True, canonical=True, g=7, seed=k + 30, out_pitch=max(1 << k, 4) + 4)
    assert workspaces_unchanged()


def extension_and_inverse_in_place(k):
    assert plan(k)["n_passes"] >= 2 and sum(plan(k)["pass_bits"]) == k
    ext = same_as_host(k, 1, n_in=1 << (k - 2), g=7, seed=k)                           # the extension: forward, shifted, a quarter of the input
    same_as_host(k, 1, inverse=True, g=pow(7, -1, R), in_place=True, seed=k + 1)
    assert ext.shape == (1, 1 << k, 4)


@pytest.mark.parametrize("k", further_pass_sizes())
def test_smallest_and_largest_size_of_every_further_pass_count(k):
    extension_and_inverse_in_place(k)


SIZES_BETWEEN = [k for k in range(P + 3, 21) if k not in further_pass_sizes()]
BIG = [21, 22, 23, 24]                                                                  # no host transform of these sizes: see "the largest sizes" below


@pytest.mark.parametrize("k", SIZES_BETWEEN)
def test_every_size_between_those(k):
    """with the two tests above: every k up to 20, so every width 2^cb of a last strided pass is run inverse with a shift"""
    extension_and_inverse_in_place(k)


def test_pass_counts_covered():
    counts = {plan(k)["n_passes"] for k in list(range(1, P + 3)) + further_pass_sizes()}
    assert counts == {plan(k)["n_passes"] for k in range(1, 21)}
    assert 1 in {b for k in range(P + 1, P + 3) for b in plan(k)["pass_bits"]}, "a one-bit pass"
    host_checked = list(range(1, P + 3)) + further_pass_sizes() + SIZES_BETWEEN            # each of them forward and, shifted, inverse
    assert sorted(host_checked + BIG) == list(range(1, 25)), "every k the call accepts, once"
    passes = lambda ks: {(j, b) for k in ks for j, b in enumerate(plan(k)["pass_bits"])}    # (which pass, how many stages)
    assert passes(host_checked + BIG) == passes(range(1, 25))
    assert {b for _, b in passes(host_checked)} == {b for _, b in passes(range(1, 25))}, "every stage count of a pass, against the host twin"
    assert {(2, 5), (2, 6)} <= passes(BIG) - passes(host_checked), "a second strided pass of 5 and of 6 stages: the largest sizes only"
    last_cb = lambda ks: {P - plan(k)["pass_bits"][-1] for k in ks if k > P}          # a strided tile is 2^cb cells wide, cb = tile bits - stages
    assert last_cb(host_checked) == last_cb(range(1, 21)) and {7, 8} <= last_cb(SIZES_BETWEEN)


# ---- three passes ---------------------------------------------------------------------------------------------------------------------------------
K3 = min(k for k in range(1, 25) if plan(k)["n_passes"] == 3)                           # two strided passes: col = blockIdx.x >> tpc in both


@pytest.mark.parametrize("form", ["columns and pitches", "pair swap with a short input", "inverse canonical"])
def test_three_passes_with_columns_pitches_and_short_inputs(form):
    n = 1 << K3
    assert K3 <= 20
    if form == "columns and pitches":
        same_as_host(K3, 3, n_in=n - 1, g=G, in_pitch=n, out_pitch=n + 4, seed=61)
    elif form == "pair swap with a short input":
        same_as_host(K3, 2, n_in=n >> 2, g=7, in_place=True, seed=62)
    else:
        same_as_host(K3, 2, inverse=True, canonical=True, g=G, out_pitch=n + 4, seed=63)
    assert workspaces_unchanged()


# ---- columns -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [min(6, PACKED), P - 1])
def test_column_counts_around_a_workgroups_share(k):
    cpg = plan(k)["cols_per_group"]
    for n_cols in sorted({1, cpg - 1, cpg, cpg + 1, 5} - {0}):
        same_as_host(k, n_cols, g=G, seed=n_cols)
        same_as_host(k, n_cols, inverse=True, in_place=True, seed=n_cols + 50, out_pitch=(1 << k) + 8)


# ---- argument forms ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [min(7, PACKED), P, P + 1])
def test_directions_limb_forms_shifts_n_in_and_placement(k):
    n = 1 << k
    t = 0
    for inverse in (False, True):
        for canonical in (False, True):
            for n_in in (1, n - 1, n >> 2, n):
                for g in (None, G):
                    in_place = bool((t // 2) & 1) if n_in != n else bool(t & 1)
                    same_as_host(k, 3, n_in=n_in, inverse=inverse, canonical=canonical, g=g, in_place=in_place, seed=t,
                                 out_pitch=n + 4 * (t % 3), in_pitch=None if in_place else ((n_in + 3) & ~3) + 8)
                    t += 1
    assert workspaces_unchanged()


# ---- round trips and sharing ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [P - 3, P + 2])
def test_forward_then_inverse_returns_the_input(k):
    cfg, n = dev_cfg(), 1 << k
    cells = columns(3, n, n, 9, False)
    d = on_device(cells)
    g, ginv = on_device(shift_of(G, False)), on_device(shift_of(pow(G, -1, R), False))
    fwd = cfg.fr_ntt(d, k, workspace=workspace(k), shift=g)
    back = cfg.fr_ntt(fwd, k, workspace=workspace(k), inverse=True, shift=ginv)
    cfg.fr_ntt(fwd, k, workspace=workspace(k), out=fwd, inverse=True, shift=ginv)          # ... and in place
    torch.cuda.synchronize()
    reduced = nr.cells_of(nr.values_of(cells, False), False).reshape(cells.shape)           # the input's elements, fully reduced
    assert np.array_equal(back.cpu().numpy().view(np.uint64), reduced) and torch.equal(back, fwd)


def test_two_workspaces_in_turn_and_one_on_two_streams():
    ka, kb = P - 2, P + 1
    for step in range(3):
        same_as_host(ka, 2, g=G, seed=step)
        same_as_host(kb, 2, inverse=True, seed=step)
    cfg, n = dev_cfg(), 1 << kb
    streams = [torch.cuda.Stream(DEV) for _ in range(2)]
    cells = [columns(2, n, n, 20 + i, False) for i in range(2)]
    d = [on_device(c) for c in cells]
    torch.cuda.synchronize()
    outs = [cfg.fr_ntt(d[i], kb, workspace=workspace(kb), inverse=bool(i), stream=streams[i]) for i in range(2)]
    for s in streams:
        s.synchronize()
    for i in range(2):
        assert np.array_equal(outs[i].cpu().numpy().view(np.uint64), _HOST.fr_ntt_host(cells[i], kb, inverse=bool(i)))
    assert workspaces_unchanged()


# ---- the largest sizes ----------------------------------------------------------------------------------------------------------------------------
# k = 21 .. 24 (coeff_to_extended of a k = 20 .. 22 circuit): pass shapes (5, 4), (5, 5), (6, 5), (6, 6) behind the 12-stage pass.  The host twin is too slow
# for them, so none of these tests runs it at 2^K: a coset decomposition into transforms of 2^20, a round trip, and Python integers at chosen outputs.
K20, N20, G0 = 20, 1 << 20, 7
_BIG = {}


def big_input():
    """(x, y0): one column of 2^20 seeded cells at a pitch of 2^20 + 8, poison above; y0 = the host twin's forward transform of size 2^20 with shift 7 —
    once per module, coset 0 of every K"""
    if not _BIG:
        x = columns(1, N20, N20 + 8, 2024, False)
        _BIG["x"], _BIG["y0"] = x, _HOST.fr_ntt_host(x, K20, n_in=N20, shift=shift_of(G0, False))
    return _BIG["x"], _BIG["y0"]


@contextlib.contextmanager
def own_workspace(k):
    """a workspace of size 2^k between guards for one test — not kept in _WS — checked unchanged when the test is through with it"""
    raw, ws = guarded(dev_cfg().fr_ntt_workspace_bytes(k) // 8, torch.int64)
    dev_cfg().fr_ntt_prepare(k, workspace=ws.view(torch.int8))
    torch.cuda.synchronize()
    keep = ws.clone()
    yield ws.view(torch.int8)
    torch.cuda.synchronize()
    assert intact(raw, ws.numel(), torch.int64) and torch.equal(ws, keep), ("the workspace", k)


@pytest.fixture
def memory_returned():
    """what a test of the largest sizes allocated goes back to the device with it, not into torch's cache"""
    yield
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.usefixtures("memory_returned")
@pytest.mark.parametrize("K", BIG)
def test_largest_sizes_are_their_cosets_of_size_2_to_the_20(K):
    """With w_K^(2^d) = w_20, d = K - 20: output 2^d j + c of the forward K-transform of x (2^20 entries, shift g0) is output j of the forward 20-transform of x
    with shift g0 w_K^c.  2^d calls at k = 20, each compared on the device; c = 0 and the last (odd) c against the host twin as well.
    Peak device memory at K = 24: 0.5 GiB the output, 0.25 GiB the table and 0.25 GiB its copy, 32 MiB each the input and ONE sub-transform: 1.1 GiB."""
    d, cfg = K - K20, dev_cfg()
    x, y0 = big_input()
    raw_in, d_in = guarded(x.size, torch.int64)
    d_in = d_in.view(1, N20 + 8, 4)
    d_in.copy_(on_device(x))
    raw_out, d_out = guarded(4 << K, torch.int64)
    d_out = d_out.view(1, 1 << K, 4)
    raw_sub, sub = guarded(4 * N20, torch.int64)
    sub = sub.view(1, N20, 4)
    with own_workspace(K) as ws:
        cfg.fr_ntt(d_in, K, workspace=ws, out=d_out, n_in=N20, shift=on_device(shift_of(G0, False)))
    assert intact(raw_out, d_out.numel(), torch.int64) and intact(raw_in, d_in.numel(), torch.int64)
    assert np.array_equal(d_in.cpu().numpy().view(np.uint64), x), "the input, and the poison above n_in"
    by_coset = d_out.view(N20, 1 << d, 4)
    for c in range(1 << d):
        g = shift_of(G0 * pow(nr.omega(K), c, R) % R, False)
        raw_sub.fill_(POISON64)
        cfg.fr_ntt(d_in, K20, workspace=workspace(K20), out=sub, n_in=N20, shift=on_device(g))
        torch.cuda.synchronize()
        assert intact(raw_sub, sub.numel(), torch.int64)
        assert torch.equal(by_coset[:, c], sub[0]), (K, c)
        if c == 0:
            assert np.array_equal(sub.cpu().numpy().view(np.uint64), y0), (K, c)
        elif c == (1 << d) - 1:
            assert np.array_equal(sub.cpu().numpy().view(np.uint64), _HOST.fr_ntt_host(x, K20, n_in=N20, shift=g)), (K, c)
    assert workspaces_unchanged()


@pytest.mark.usefixtures("memory_returned")
@pytest.mark.parametrize("K", BIG)
def test_largest_sizes_forward_then_inverse_in_place(K):
    """A dense column of 2^K random reduced cells (two columns at K = 21), forward in place with G, inverse in place with 1 / G: the column again.
    Peak device memory at K = 24: 0.5 GiB each the column, its copy and the random draw, 0.25 GiB the table and 0.25 GiB its copy: 2 GiB."""
    cfg, n, n_cols = dev_cfg(), 1 << K, 2 if K == 21 else 1
    raw, d = guarded(n_cols * n * 4, torch.int64)
    d = d.view(n_cols, n, 4)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(K)
    d.copy_(torch.randint(0, 1 << 62, (n_cols, n, 4), dtype=torch.int64, device=DEV, generator=gen))
    d[:, :, 3] >>= 2                                                                       # below 2^252 < r
    keep = d.clone()
    g, ginv = on_device(shift_of(G, False)), on_device(shift_of(pow(G, -1, R), False))
    with own_workspace(K) as ws:
        assert cfg.fr_ntt(d, K, workspace=ws, out=d, shift=g).data_ptr() == d.data_ptr()
        torch.cuda.synchronize()
        assert not torch.equal(d, keep) and bool((d[:, :, 3] >> 62 == 0).all())           # transformed, every cell below 2^254
        cfg.fr_ntt(d, K, workspace=ws, out=d, inverse=True, shift=ginv)
    assert torch.equal(d, keep) and intact(raw, d.numel(), torch.int64)


@pytest.mark.usefixtures("memory_returned")
@pytest.mark.parametrize("K", BIG)
def test_largest_sizes_against_python_integers_around_every_pass_border(K):
    """n_in = 64 and shift G: both directions, both limb forms, about 40 outputs each against Horner evaluation in Python integers —
    forward y[j] = x(G w_K^j); inverse y[i] = G^i 2^-K x(w_K^-i) — at 0, 1, 2^K - 1, 2^(K-1) +- 1, 4095 .. 4097, around 2^s0 of every pass and 24 seeded ones.
    Peak device memory at K = 24: 0.5 GiB the output, 0.25 GiB the table and 0.25 GiB its copy: 1 GiB."""
    cfg, n, n_in = dev_cfg(), 1 << K, 64
    starts = np.cumsum([0] + plan(K)["pass_bits"][:-1])                                    # s0 of every pass
    idx = {0, 1, n - 1, n // 2 - 1, n // 2 + 1, 4095, 4096, 4097} | {(1 << int(s0)) + e for s0 in starts for e in (-1, 0, 1)}
    idx = sorted(idx | {int(i) for i in np.random.default_rng(K).integers(0, n, 24)})
    assert len(starts) == 3 and 30 <= len(idx) <= 45
    w, winv, ninv = nr.omega(K), pow(nr.omega(K), -1, R), pow(n, -1, R)
    raw, d_out = guarded(4 * n, torch.int64)
    d_out = d_out.view(1, n, 4)
    pick = torch.tensor(idx, device=DEV)
    with own_workspace(K) as ws:
        for inverse in (False, True):
            for canonical in (False, True):
                cells = columns(1, n_in, n_in, 70 + 2 * inverse + canonical, canonical)
                x = nr.values_of(cells[0], canonical)
                raw.fill_(POISON64)
                cfg.fr_ntt(on_device(cells), K, workspace=ws, out=d_out, inverse=inverse, n_in=n_in, shift=on_device(shift_of(G, canonical)), canonical=canonical)
                torch.cuda.synchronize()
                assert intact(raw, d_out.numel(), torch.int64) and bool((d_out[0, :, 3] != POISON64).all()), "every entry below 2^K written"
                got = nr.values_of(d_out[0, pick].cpu().numpy().view(np.uint64), canonical)
                if inverse:
                    want = [pow(G, i, R) * ninv * nr.eval_at(x, pow(winv, i, R)) % R for i in idx]
                else:
                    want = [nr.eval_at(x, G * pow(w, j, R) % R) for j in idx]
                assert got == want, (K, inverse, canonical, [i for i, a, b in zip(idx, got, want) if a != b])


# ---- the chain -------------------------------------------------------------------------------------------------------------------------------------
def test_lookup_columns_to_coefficients_and_to_the_extended_coset():
    M, B, n_rows, pitch, k = 64, 3, 4090, 4096, 12
    cfg = dev_cfg()
    chars, lens = batch(B, M, seed=5)
    d_chars, d_lens = torch.from_numpy(chars).to(DEV), torch.from_numpy(lens.astype(np.int32)).to(DEV)
    ch = challenges(3, 13, False)
    theta, beta, gamma = (on_device(c) for c in ch)
    rec = cfg.witness_batch(d_chars, d_lens)[0]
    counts, misses = cfg.lookup_counts(d_chars, d_lens, rec)
    table, inputs = cfg.lookup_compress_table(theta)[0], cfg.lookup_compress_inputs(d_chars, d_lens, rec, theta)
    perm = cfg.lookup_permute(counts, n_rows, table=table, pitch=pitch)
    ib, ig = cfg.lookup_invert_table(table, beta), cfg.lookup_invert_table(table, gamma)
    z = cfg.lookup_product(d_lens, inputs, perm["a_idx"], perm["s_idx"], n_rows, table, ib, ig, beta, gamma, z_pitch=pitch)["z"]
    cols = {"a": perm["a_cells"], "s": perm["s_cells"], "z": z}
    blind = on_device(nr.cells_of([int(v) * 0x9e3779b97f4a7c15 % R for v in range(1, pitch - n_rows + 1)], False))      # the rows above n_rows are the caller's
    lagrange = {}
    for name, t in cols.items():
        assert tuple(t.shape) == (3, B, pitch, 4)
        first = n_rows + (1 if name == "z" else 0)
        t[:, :, first:] = blind[:pitch - first]
        lagrange[name] = t.cpu().numpy().view(np.uint64).copy()
        flat = t.view(3 * B, pitch, 4)
        assert cfg.fr_ntt(flat, k, workspace=workspace(k), out=flat, inverse=True).data_ptr() == t.data_ptr()       # lagrange_to_coeff, in place
    torch.cuda.synchronize()
    w = nr.omega(k)
    rows = [0, 1, 2, 63, 64, 65, 1023, 1024, 2047, 2048, 3000, n_rows - 1, n_rows, n_rows + 1, pitch - 2, pitch - 1]
    for name, t in cols.items():
        coeffs = t.cpu().numpy().view(np.uint64)
        assert np.array_equal(coeffs.reshape(3 * B, pitch, 4), _HOST.fr_ntt_host(lagrange[name].reshape(3 * B, pitch, 4), k, inverse=True)), name
        for c in range(3):
            for b in range(B):
                co = nr.values_of(coeffs[c, b], False)
                want = nr.values_of(lagrange[name][c, b][rows], False)
                assert [nr.eval_at(co, pow(w, i, R)) for i in rows] == want, (name, c, b)
    # coeff_to_extended: forward at k + 2 over the 4096 coefficients, on the coset of 7
    ke = k + 2
    seven = shift_of(7, False)
    raw, ext = guarded(3 * B * (1 << ke) * 4, torch.int64)
    ext = ext.view(3 * B, 1 << ke, 4)
    cfg.fr_ntt(cols["z"].view(3 * B, pitch, 4), ke, workspace=workspace(ke), out=ext, n_in=pitch, shift=on_device(seven))
    torch.cuda.synchronize()
    want = _HOST.fr_ntt_host(cols["z"].cpu().numpy().view(np.uint64).reshape(3 * B, pitch, 4), ke, n_in=pitch, shift=seven)
    assert np.array_equal(ext.cpu().numpy().view(np.uint64), want) and intact(raw, ext.numel(), torch.int64)
    co = nr.values_of(cols["z"][0, 0].cpu().numpy().view(np.uint64), False)
    for j in (0, 1, (1 << ke) - 1):                                                        # ... which is the polynomial on 7 w_14^j
        assert nr.values_of(ext[0, j].cpu().numpy().view(np.uint64), False)[0] == nr.eval_at(co, 7 * pow(nr.omega(ke), j, R) % R)


# ---- the contract ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [PACKED, P, P + 2])
def test_capture_replay_as_the_first_calls_of_a_fresh_context_and_a_side_stream(k):
    n = 1 << k
    cells = columns(3, n >> 2, n >> 2, 4, False)
    shift = shift_of(G, False)
    want = _HOST.fr_ntt_host(cells, k, n_in=n >> 2, shift=shift)
    cfg = hra.RegexVerifyConfig.configure(64, defs_of_files(CFG_1), device=0)             # no call of any kind on it before the capture
    d_in, d_shift = on_device(cells), on_device(shift)
    raw_ws, ws = guarded(cfg.fr_ntt_workspace_bytes(k) // 8, torch.int64)
    raw, out = guarded(3 * n * 4, torch.int64)
    out = out.view(3, n, 4)
    side = torch.cuda.Stream(DEV)

    def run(stream):
        cfg.fr_ntt_prepare(k, workspace=ws.view(torch.int8), stream=stream)
        cfg.fr_ntt(d_in, k, workspace=ws.view(torch.int8), out=out, n_in=n >> 2, shift=d_shift, stream=stream)

    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        run(side)
    torch.cuda.synchronize()
    assert bool((raw == POISON64).all()) and bool((raw_ws == POISON64).all())                 # captured, not run
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint64), want) and intact(raw, out.numel(), torch.int64) and intact(raw_ws, ws.numel(), torch.int64)
        raw.fill_(POISON64)
    run(side)                                                                               # eager, on the side stream
    side.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want)


def test_two_contexts_in_turn():
    cfgs = [hra.RegexVerifyConfig.configure(64, defs_of_files(names), device=0) for names in (CFG_1, CFG_23)]
    ks = (PACKED - 1, P + 1)
    wss = [[c.fr_ntt_prepare(k) for k in ks] for c in cfgs]
    for step in range(2):
        for i, c in enumerate(cfgs):
            for j, k in enumerate(ks):
                same_as_host(k, 2, inverse=bool(step), g=G, seed=10 * step + i, cfg=c, ws=wss[i][j])
                same_as_host(k, 2, inverse=bool(step), g=G, seed=10 * step + i, cfg=c, ws=wss[1 - i][j])      # a workspace serves every context of the device


def test_refused_calls_write_nothing():
    cfg, k, n = dev_cfg(), 6, 64
    ctx, ws = cfg._need_ctx(), workspace(k)
    raw_in, d_in = guarded(3 * n * 2 * 4, torch.int64)
    raw, d_out = guarded(3 * n * 2 * 4, torch.int64)
    d_shift = on_device(shift_of(7, False))
    inp, outp, sp, wp, wb = d_in.data_ptr(), d_out.data_ptr(), d_shift.data_ptr(), ws.data_ptr(), ws.numel()
    s = torch.cuda.current_stream(DEV).cuda_stream
    INV, CAN = hra.FR_NTT_INVERSE, hra.FR_CANONICAL
    dev = lambda *a: hra.lib.hrx_fr_ntt_device(ctx, *a)
    bad = {
        "NULL in": (None, n, outp, n, 3, k, n, sp, 0, wp, wb), "NULL out": (inp, n, None, n, 3, k, n, sp, 0, wp, wb),
        "misaligned in": (inp + 8, n, outp, n, 3, k, n, sp, 0, wp, wb), "misaligned out": (inp, n, outp + 8, n, 3, k, n, sp, 0, wp, wb),
        "misaligned shift": (inp, n, outp, n, 3, k, n, sp + 4, 0, wp, wb),
        "k = 0": (inp, n, outp, n, 3, 0, 1, sp, 0, wp, wb), "k = 25": (inp, n, outp, n, 3, 25, n, sp, 0, wp, wb),
        "n_in = 0": (inp, n, outp, n, 3, k, 0, sp, 0, wp, wb), "n_in above 2^k": (inp, n + 4, outp, n + 4, 3, k, n + 1, sp, 0, wp, wb),
        "in_pitch below n_in": (inp, n - 4, outp, n, 3, k, n, sp, 0, wp, wb), "in_pitch no multiple of 4": (inp, n + 2, outp, n, 3, k, n, sp, 0, wp, wb),
        "out_pitch below 2^k": (inp, n, outp, n - 4, 3, k, n - 4, sp, 0, wp, wb), "out_pitch no multiple of 4": (inp, n, outp, n + 1, 3, k, n, sp, 0, wp, wb),
        "unknown flag": (inp, n, outp, n, 3, k, n, sp, 4, wp, wb), "unknown flags": (inp, n, outp, n, 3, k, n, sp, INV | CAN | 8, wp, wb),
        "overlap, shifted": (outp + 32, n, outp, n, 3, k, n, sp, 0, wp, wb), "overlap, other pitch": (outp, n, outp, n + 4, 3, k, n, sp, 0, wp, wb),
        "overlap, out inside in": (outp, n, outp + 32 * n, n, 3, k, n, sp, 0, wp, wb),
        "no workspace": (inp, n, outp, n, 3, k, n, sp, 0, None, wb), "misaligned workspace": (inp, n, outp, n, 3, k, n, sp, 0, wp + 128, wb),
        "small workspace": (inp, n, outp, n, 3, k, n, sp, 0, wp, wb - 1), "the workspace of a smaller k": (inp, 2 * n, outp, 2 * n, 3, k + 1, 2 * n, sp, 0, wp, wb),
    }
    for what, args in bad.items():
        assert dev(*args, s) == hra.HRX_ERR_ARG, what
    for what, args in {"no workspace": (k, None, wb), "misaligned": (k, wp + 128, wb), "small": (k, wp, wb - 1), "k = 0": (0, wp, wb), "k = 25": (25, wp, 1 << 40)}.items():
        assert hra.lib.hrx_fr_ntt_prepare_device(ctx, *args, s) == hra.HRX_ERR_ARG, what
    assert dev(inp, n, outp, n, 0, k, n, sp, 0, wp, wb, s) == hra.HRX_OK                    # no columns: nothing launched
    torch.cuda.synchronize()
    assert bool((raw == POISON64).all()) and bool((raw_in == POISON64).all()) and workspaces_unchanged()
    host_only = _HOST._need_ctx()
    assert hra.lib.hrx_fr_ntt_device(host_only, inp, n, outp, n, 3, k, n, sp, 0, wp, wb, s) == hra.HRX_ERR_HIP
    assert hra.lib.hrx_fr_ntt_prepare_device(host_only, k, wp, wb, s) == hra.HRX_ERR_HIP
