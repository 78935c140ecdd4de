"""LOOKUP QUOTIENT on the device (include/hrx.h hrx_fr_vanishing_inverse_device / hrx_lookup_quotient_device; csrc/hrx_kernel_quotient.hip) against the host
twin (which test_quotient_cpu.py holds against Python integers), every limb, every buffer between poisoned guards:
  small sizes      every (k, e) with k in 1..6 and e in 1..3 at 3 D = 3, 1 and 3 strings: columns shorter than a tile, and shorter than the halo's reach
  tile borders     N in {tile / 2, tile, 2 tile} of lookup_quotient_plan with e = 1 and e = 6: the rotated reads cross the tile border — and wrap around the
                   column's ends — by 2 cells and by 64
  defs             regex2 + regex3 (3 D = 6)
  argument forms   both limb forms, both strides of every kind, h_in NULL, apart and in place, four different pitches with the tails poisoned, the inputs
                   unchanged, the division on and off
  the table        fr_vanishing_inverse on the device against the host
  the chain        regex1's device stages at pitch 4096, the transforms to the coset of ZETA at k = 14, the quotient: the host twin's cells, and zero modulo
                   X^n - 1 (the inverse transform on the device, the fold in Python integers at 64 sampled rows)
  contract         capture and replay as a fresh context's first call, a side stream, every refusal with nothing written, a host-only context"""
import gc
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import halo2_regex_amd as hra
import ntt_ref as nr
from compress_ref import R
from test_compress_gpu import on_device
from test_match_cpu import CFG_1, CFG_23
from test_permute_gpu import guarded, intact, POISON64
from test_quotient_cpu import Case, H_MODES, K, EXT_K, N_ROWS, SIZES, cfg_of, folded, host_chain, refusals, shift_limbs
from test_verify_gpu import defs_of_files

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TILE = cfg_of(3).lookup_quotient_plan(1, 10)["tile_cells"]
_CFG = {}


@pytest.fixture(scope="module", autouse=True)
def release_the_shared_contexts():
    """the module's device contexts go with the module: a device's placement arenas live as long as any context on it does, and later modules count on
    starting without one"""
    yield
    _CFG.clear()
    gc.collect()


def dev_cfg(ncols=3):
    if ncols not in _CFG:
        _CFG[ncols] = hra.RegexVerifyConfig.configure(64, defs_of_files({3: CFG_1, 6: CFG_23}[ncols]), device=0)
    return _CFG[ncols]


def upload(a):
    """a numpy array of limbs on the device between guards: (raw, tensor of a's shape)"""
    raw, t = guarded(a.size, torch.int64)
    t = t.view(a.shape)
    t.copy_(on_device(a))
    return raw, t


def same_as_host(case, cfg=None, stream=None):
    """one device call on the case's arrays between guards against the host twin on the same arrays: the cells, the pitch tails, the guards, the inputs"""
    cfg = cfg or dev_cfg(case.ncols)
    want = cfg_of(case.ncols).lookup_quotient_host(**case.call_args(h_in=case.h_in))
    dev = {name: upload(a) for name, a in case.arrays.items()}
    ch = [upload(c) for c in case.challenges]
    t_inv = upload(case.t_inv) if case.t_inv is not None else None
    if case.h_mode == "none":
        h_in = None
    raw_out, out = guarded(case.b_count * case.h_pitch * 4, torch.int64)
    out = out.view(case.b_count, case.h_pitch, 4)
    if case.h_mode == "in place":
        out.copy_(on_device(case.h_in))
        h_in = out
    elif case.h_mode == "separate":
        raw_h, h_in = upload(case.h_in)
    res = cfg.lookup_quotient(case.k, case.ext_k, dev["A"][1], dev["Ap"][1], dev["Sp"][1], dev["Z"][1], dev["S"][1], dev["sel"][1], ch[0][1], ch[1][1], ch[2][1],
                              h_in=h_in, out=out, t_inv=t_inv[1] if t_inv else None, divide=case.divide, canonical=case.canonical, stream=stream)
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    assert res.data_ptr() == out.data_ptr()
    got = out.cpu().numpy().view(np.uint64)
    what = (case.k, case.ext_k, case.ncols, case.b_count, case.canonical, case.h_mode, case.divide)
    assert np.array_equal(got[:, :case.N], want[:, :case.N]), what
    tail = case.h_in[:, case.N:] if case.h_mode == "in place" else POISON64
    assert (got[:, case.N:] == tail).all() and intact(raw_out, out.numel(), torch.int64), what
    for name, (raw, t) in dev.items():
        assert intact(raw, t.numel(), torch.int64) and np.array_equal(t.cpu().numpy().view(np.uint64), case.arrays[name]), (what, name)
    if case.h_mode == "separate":
        assert np.array_equal(h_in.cpu().numpy().view(np.uint64), case.h_in) and intact(raw_h, h_in.numel(), torch.int64)
    return got


def forms(j):
    return dict(canonical=bool(j & 1), per_string=bool(j & 2), s_stride=(j >> 2) & 1, h_mode=H_MODES[j % 3], divide=bool((j >> 3) & 1) != bool(j & 1))


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,ke", list(enumerate(SIZES)))
def test_small_sizes(i, ke):
    k, e = ke
    same_as_host(Case(3, k, e, 1, seed=i + 1, **forms(i)))
    same_as_host(Case(3, k, e, 3, seed=i + 31, **forms(i + 7)))


@pytest.mark.parametrize("e", [1, 6])
@pytest.mark.parametrize("N", [TILE // 2, TILE, 2 * TILE])
def test_around_the_tile(N, e):
    ext_k = N.bit_length() - 1
    assert 1 << ext_k == N and ext_k - e >= 1
    for j, b_count in enumerate((1, 3)):
        same_as_host(Case(3, ext_k - e, e, b_count, seed=ext_k * 10 + e + j, **forms(ext_k + e + 5 * j)))
    same_as_host(Case(3, ext_k - e, e, 2, seed=ext_k + e, **forms(ext_k + e + 8)))


def test_six_lookups():
    for j, (k, e, b_count) in enumerate([(2, 1, 3), (5, 2, 2), (TILE.bit_length() - 2, 2, 1), (4, 6, 3)]):
        same_as_host(Case(6, k, e, b_count, seed=60 + j, **forms(3 * j + 1)))


@pytest.mark.parametrize("canonical", [False, True])
def test_every_argument_form(canonical):
    seed = 200
    for per_string, s_stride, h_mode, divide in itertools.product((False, True), (0, 1), H_MODES, (False, True)):
        seed += 1
        same_as_host(Case(3, 4, 2, 3, canonical, per_string, s_stride, h_mode, divide, seed))
    same_as_host(Case(3, 3, 2, 2, canonical, True, 1, "separate", True, seed=9, unreduced=True))      # challenges of r and more are taken mod r first


# ---- the vanishing inverse -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [False, True])
def test_vanishing_inverse_against_the_host(canonical):
    cfg = dev_cfg()
    for k, e in [(1, 1), (1, 6), (3, 2), (12, 2), (18, 6), (23, 1)]:
        for g in (7, nr.ZETA, nr.ZETA * nr.ZETA % R, 1):
            shift = shift_limbs(g, canonical)
            raw, out = guarded((1 << e) * 4, torch.int64)
            res = cfg.fr_vanishing_inverse(k, k + e, on_device(shift), out=out.view(1 << e, 4), canonical=canonical)
            torch.cuda.synchronize()
            assert res.data_ptr() == out.data_ptr() and intact(raw, out.numel(), torch.int64)
            want = cfg_of(3).fr_vanishing_inverse_host(k, k + e, shift, canonical=canonical)
            assert np.array_equal(out.view(1 << e, 4).cpu().numpy().view(np.uint64), want), (k, e, g)
    none = cfg.fr_vanishing_inverse(3, 5, canonical=canonical)
    torch.cuda.synchronize()
    assert np.array_equal(none.cpu().numpy().view(np.uint64), cfg_of(3).fr_vanishing_inverse_host(3, 5, shift_limbs(1, canonical), canonical=canonical))


# ---- the chain -------------------------------------------------------------------------------------------------------------------------------------------
def test_the_chain_on_the_device():
    """the honest strings of the host chain through the device stages at pitch 4096, to the coset of ZETA at k = 14, through the quotient"""
    hc = host_chain(False)
    cfg, hch, n, N, pitch = dev_cfg(), hc["ch"], 1 << K, 1 << EXT_K, 1 << K
    B, M = hch.B, hch.M
    d_chars, d_lens = torch.from_numpy(hc["chars"]).to(DEV), torch.from_numpy(hc["lens"].astype(np.int32)).to(DEV)
    theta, beta, gamma, y = (on_device(c) for c in (hch.theta, hch.beta, hch.gamma, hc["y"]))
    rec = cfg.witness_batch(d_chars, d_lens)[0]
    counts, misses = cfg.lookup_counts(d_chars, d_lens, rec)
    table, inputs = cfg.lookup_compress_table(theta)[0], cfg.lookup_compress_inputs(d_chars, d_lens, rec, theta)
    perm = cfg.lookup_permute(counts, N_ROWS, table=table, pitch=pitch)
    ib, ig = cfg.lookup_invert_table(table, beta), cfg.lookup_invert_table(table, gamma)
    prod = cfg.lookup_product(d_lens, inputs, perm["a_idx"], perm["s_idx"], N_ROWS, table, ib, ig, beta, gamma, z_pitch=pitch)
    assert not misses.cpu().numpy().any() and not prod["open"].cpu().numpy().any()         # honest strings: the argument closes
    blind = on_device(nr.cells_of([int(v) * 0x9e3779b97f4a7c15 % R for v in range(1, pitch + 1)], False))      # the rows above n_rows are the caller's
    A = torch.empty((3, B, pitch, 4), dtype=torch.int64, device=DEV)
    S = torch.empty((3, pitch, 4), dtype=torch.int64, device=DEV)
    lay = cfg.lookup_layout()
    for c in range(3):                                                                     # A[r], S[r] by LOOKUP PRODUCT's definition
        sl = lay[0][("trans", "start", "end")[c]]
        S[c] = table[sl.start]
        S[c, :sl.stop - sl.start] = table[sl]
        for b in range(B):
            nb = int(hc["lens"][b])
            A[c, b] = table[sl.start]
            if nb <= M:
                rows = M - 1 if (nb == M and c != 1) else M
                A[c, b, :rows] = inputs[c, b, :rows]
    cols = {"A": A, "Ap": perm["a_cells"], "Sp": perm["s_cells"], "Z": prod["z"]}
    for name, t in cols.items():
        first = N_ROWS + (1 if name == "Z" else 0)
        t[:, :, first:] = blind[:pitch - first]
    ws_k, ws_ext = cfg.fr_ntt_prepare(K), cfg.fr_ntt_prepare(EXT_K)
    zeta, zeta_inv = on_device(shift_limbs(nr.ZETA, False)), on_device(shift_limbs(pow(nr.ZETA, -1, R), False))

    def to_coset(t):
        flat = t.view(-1, pitch, 4)
        cfg.fr_ntt(flat, K, workspace=ws_k, out=flat, inverse=True)
        return cfg.fr_ntt(flat, EXT_K, workspace=ws_ext, n_in=pitch, shift=zeta).view(tuple(t.shape[:-2]) + (N, 4))

    ext = {name: to_coset(t) for name, t in cols.items()}
    s_ext = to_coset(S)
    sel = cfg.lookup_quotient_selectors(K, EXT_K, N_ROWS, zeta, device=DEV, workspaces=(ws_k, ws_ext))
    raw, h = guarded(B * N * 4, torch.int64)
    h = h.view(B, N, 4)
    cfg.lookup_quotient(K, EXT_K, ext["A"], ext["Ap"], ext["Sp"], ext["Z"], s_ext, sel, beta, gamma, y, out=h)
    torch.cuda.synchronize()
    host = lambda t: t.cpu().numpy().view(np.uint64)
    assert np.array_equal(host(sel), hc["sel"])
    want = cfg_of(3).lookup_quotient_host(K, EXT_K, host(ext["A"]), host(ext["Ap"]), host(ext["Sp"]), host(ext["Z"]), host(s_ext), host(sel), hch.beta, hch.gamma,
                                          hc["y"])
    assert np.array_equal(host(h), want) and intact(raw, h.numel(), torch.int64)
    coeff = host(cfg.fr_ntt(h, EXT_K, workspace=ws_ext, inverse=True, shift=zeta_inv))
    edge = [0, 1, n - 1, N_ROWS - 1, N_ROWS, N_ROWS + 1]
    rows = edge + [int(i) for i in np.random.default_rng(4).permutation(n) if int(i) not in edge][:58]      # 64 sampled rows
    for b in range(B):
        sample = np.concatenate([coeff[b, [i + c * n for c in range(N // n)]] for i in rows])
        vals = nr.values_of(sample, False)
        assert any(vals) and [sum(vals[4 * j:4 * j + 4]) % R for j in range(len(rows))] == [0] * len(rows), b


# ---- the contract ----------------------------------------------------------------------------------------------------------------------------------------
def test_capture_replay_as_the_first_call_of_a_fresh_context_and_a_side_stream():
    case = Case(3, 7, 2, 3, True, True, 1, "separate", True, seed=77)
    want = cfg_of(3).lookup_quotient_host(**case.call_args(h_in=case.h_in))
    cfg = hra.RegexVerifyConfig.configure(64, defs_of_files(CFG_1), device=0)             # no call of any kind on it before the capture
    dev = {name: on_device(a) for name, a in case.arrays.items()}
    ch = [on_device(c) for c in case.challenges]
    h_in, shift = on_device(case.h_in), on_device(shift_limbs(case.g, True))
    raw_t, t_inv = guarded((1 << 2) * 4, torch.int64)
    raw, out = guarded(case.b_count * case.h_pitch * 4, torch.int64)
    out = out.view(case.b_count, case.h_pitch, 4)
    side = torch.cuda.Stream(DEV)

    def run(stream):
        cfg.fr_vanishing_inverse(case.k, case.ext_k, shift, out=t_inv.view(4, 4), canonical=True, stream=stream)
        cfg.lookup_quotient(case.k, case.ext_k, dev["A"], dev["Ap"], dev["Sp"], dev["Z"], dev["S"], dev["sel"], ch[0], ch[1], ch[2], h_in=h_in, out=out,
                            t_inv=t_inv.view(4, 4), divide=True, canonical=True, stream=stream)

    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        run(side)
    torch.cuda.synchronize()
    assert bool((raw == POISON64).all()) and bool((raw_t == POISON64).all())                  # captured, not run
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint64)
        assert np.array_equal(got[:, :case.N], want[:, :case.N]) and (got[:, case.N:] == POISON64).all()
        assert intact(raw, out.numel(), torch.int64) and intact(raw_t, t_inv.numel(), torch.int64)
        raw.fill_(POISON64)
    run(side)                                                                               # eager, on the side stream
    side.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64)[:, :case.N], want[:, :case.N])


def test_refused_calls_write_nothing():
    k, e, b, ncols = 3, 2, 2, 3
    N = 1 << (k + e)
    cfg = dev_cfg()
    ctx = cfg._need_ctx()
    cells = ncols * b * (N + 16) * 4
    bufs = {n: guarded(cells, torch.int64) for n in ("a", "ap", "sp", "z", "s", "sel", "h_in", "t", "h_out")}
    bufs.update({n: guarded(b * 4, torch.int64) for n in ("beta", "gamma", "y")})
    for n, (raw, t) in bufs.items():
        if n != "h_out":
            t.zero_()
    ptr = {n: t.data_ptr() for n, (raw, t) in bufs.items()}
    good, bad, with_ = refusals(k, e, b, ncols, ptr)
    s = torch.cuda.current_stream(DEV).cuda_stream
    dev = lambda *a: hra.lib.hrx_lookup_quotient_device(ctx, *a, s)
    for what, args in bad.items():
        assert dev(*args) == hra.HRX_ERR_ARG, what
    assert dev(*with_(b_count=0)) == hra.HRX_OK                                            # no strings: nothing launched
    tp, sp = ptr["h_out"], ptr["beta"]
    for what, args in {"NULL t_inv": (k, k + e, sp, None, 0), "misaligned t_inv": (k, k + e, sp, tp + 8, 0), "misaligned shift": (k, k + e, sp + 4, tp, 0),
                       "k = 0": (0, e, sp, tp, 0), "e = 0": (k, k, sp, tp, 0), "e = 7": (k, k + 7, sp, tp, 0), "ext_k = 25": (24, 25, sp, tp, 0),
                       "unknown flag": (k, k + e, sp, tp, 2)}.items():
        assert hra.lib.hrx_fr_vanishing_inverse_device(ctx, *args, s) == hra.HRX_ERR_ARG, what
    torch.cuda.synchronize()
    assert bool((bufs["h_out"][0] == POISON64).all())
    host_only = cfg_of(3)._need_ctx()
    assert hra.lib.hrx_lookup_quotient_device(host_only, *good, s) == hra.HRX_ERR_HIP
    assert hra.lib.hrx_fr_vanishing_inverse_device(host_only, k, k + e, sp, tp, 0, s) == hra.HRX_ERR_HIP
    torch.cuda.synchronize()
    assert bool((bufs["h_out"][0] == POISON64).all())
    assert dev(*good) == hra.HRX_OK                                                        # ... and the good call is one
    torch.cuda.synchronize()
    assert intact(bufs["h_out"][0], cells, torch.int64) and not bool((bufs["h_out"][1] == POISON64).all())
