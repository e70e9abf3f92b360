"""The BatchNorm kernels at training scale, against float64 references computed from exactly the values the kernels read:
``K.bn_fwd`` / ``K.bn_bwd`` (csrc/bn.hip, the wide-channel BatchNorm + ReLU of unet_bn) and the Enet family (csrc/enet.hip:
``K.enet_bn_fwd_stats``, ``K.enet_bn_bwd``, its split form, the statistics rows the MFMA convolutions write and the data-gradient
convolution that applies the BatchNorm backward on load).

Both families make per-block partial sums (fp32 runs flushed into doubles), cap the grid at 256 blocks, fold the partials in a fixed
order in double and take the variance in one pass as s2 / count - mean^2.  The pixel counts here cross the grid caps with ragged last
blocks, and the statistics carry *sentinel* pixels at the first and last pixel of blocks and at the last pixel of the ragged block,
each worth far more than the bound, so a kernel that loses or double-counts one pixel fails.  Every output is pre-filled with NaN, or
with known values where the kernel adds to it.

Error model (U = 2^-24, the fp32 unit roundoff; first order, with 1 % slack for the second-order terms):
  * an fp32 running sum of at most RUN terms (bn.hip: 64 pixels, enet.hip: 32 pixels; the MFMA epilogue sums a 32-pixel tile) is off
    by at most (RUN - 1) U sum|terms|; the doubles that collect the runs and fold the partials add FOLD = 2^-53 * 4096 relative to
    sum|terms| (a fold chain is far shorter than 4096 adds).  So |s - S| <= (RUN U + FOLD) sum|terms| for every per-channel sum;
  * the variance s2 / n - m^2 is then off by ds2 / n + 2 |m| dm: the one-pass form's cancellation is in this bound, which grows with
    (|mean| / std)^2 relative to the variance;
  * every fp32 operation after that adds one rounding (U relative to its result), a bf16 store half a bf16 ulp (2^-8 relative).
The references are computed in float64 on the device from the tensors the kernels read (bf16 inputs are quantised first)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24                  # fp32 unit roundoff
UB = 2.0 ** -8                  # bf16 unit roundoff (half an ulp, relative)
FOLD = 2.0 ** -53 * 4096        # the double collection and fold of the fp32 runs, relative to sum|terms|
TINY = 2.0 ** -120              # absolute floor: results near fp32's smallest normals
SLACK = 1.01                    # second-order terms of the first-order bounds
RUN_BN = 64                     # bn.hip bn_reduce_kernel: fp32 runs of 64 pixels
RUN_ENET = 32                   # enet.hip ReduceVecK (runs of 32 pixels), MFMA epilogue (tiles of 32 pixels); ReduceK sums in double
EPS_BN, EPS_ENET, MOM = 1e-5, 1e-3, 0.1


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dct_amd import hip_ops
    return hip_ops


# ------------------------------------------------------------------------------------------------ grid plans (mirrors of the C code)
def bn_plan(P, C):
    """csrc/bn.hip plan_blocks: >= 16 pixels per thread, at most BN_MAX_BLOCKS = 256 blocks -> (ppb, blocks)."""
    rows = 256 // (C // 8)
    blocks = min(max(-(-P // (16 * rows)), 1), 256)
    ppb = -(-P // blocks)
    return ppb, -(-P // ppb)


def bn_cap(C):
    """The pixel count at which plan_blocks reaches its 256-block cap."""
    return 256 * 16 * (256 // (C // 8))


def enet_plan(P, C):
    """csrc/enet.hip red_plan: g_enet_reduce_ppt = 8 pixels per thread, rows = 256 / next_pow2(C), at most 256 blocks."""
    cp = 1 << max(C - 1, 0).bit_length()
    rows = 256 // cp
    blocks = min(max(-(-P // (8 * rows)), 1), 256)
    ppb = -(-P // blocks)
    return ppb, -(-P // ppb)


def enet_cap(C):
    return 256 * 8 * (256 // (1 << max(C - 1, 0).bit_length()))


def sentinel_pixels(P, ppb, blocks):
    """First pixel of a block, last pixel of a block, first and last pixel of the (ragged) last block."""
    cand = {0, ppb - 1, ppb, 2 * ppb - 1, (blocks // 2) * ppb, (blocks - 1) * ppb, P - 1}
    return sorted(i for i in cand if 0 <= i < P)


# ------------------------------------------------------------------------------------------------ data
def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def raw_like(g, P, C, dt, ratio=None, sentinels=()):
    """[P, C] raw conv outputs: per channel mean mu_c and spread s_c (``ratio``: |mu_c| / s_c fixed), rounded to ``dt``; sentinel pixels
    get mu_c + (0.5 + 0.1 j) sqrt(P) s_c -- losing one moves the mean by ~0.5 s_c / sqrt(P), far more than its bound."""
    s = torch.rand(C, generator=g, device=DEV) * 1.5 + 0.5
    if ratio is None:
        mu = (torch.rand(C, generator=g, device=DEV) * 4 - 2) * s
    else:
        mu = ratio * s * torch.where(torch.rand(C, generator=g, device=DEV) < 0.5, -1.0, 1.0)
    x = torch.randn(P, C, generator=g, device=DEV) * s + mu
    for j, pix in enumerate(sentinels):
        x[pix] = mu + (0.5 + 0.1 * j) * math.sqrt(P) * s
    return x.to(dt)


def grad_like(g, P, C, dt, sentinels=()):
    x = torch.randn(P, C, generator=g, device=DEV)
    for j, pix in enumerate(sentinels):
        x[pix] = (0.5 + 0.1 * j) * math.sqrt(P)
    return x.to(dt)


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def nhwc(flat, shape):
    return flat.view(*shape, flat.shape[-1])


def check(got, ref, bound, what):
    """|got - ref| <= bound elementwise, in float64; NaN anywhere in got fails."""
    got = got.detach().double()
    ref, bound = torch.as_tensor(ref, dtype=torch.float64, device=got.device), torch.as_tensor(bound, dtype=torch.float64, device=got.device)
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    err = (got - ref).abs()
    bad = ~(err <= bound)
    if bad.any():
        i = int(torch.nonzero(bad.reshape(-1))[0])
        b = bound.expand_as(err).reshape(-1)[i].item()
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} out of bound; first at flat {i}: got {got.reshape(-1)[i].item()!r} "
                             f"ref {ref.reshape(-1)[i].item()!r} bound {b!r}")


# ------------------------------------------------------------------------------------------------ references and bounds
def stats_ref(x64, run):
    """Batch mean / biased variance (two-pass, float64) of x64 [P, C] and the bounds dm, dv of the kernels' one-pass double values."""
    P = x64.shape[0]
    m = x64.sum(0) / P
    v = ((x64 - m) ** 2).sum(0) / P
    k = run * U + FOLD
    dm = k * x64.abs().sum(0) / P * SLACK
    dv = (k * (x64 * x64).sum(0) / P + 2 * m.abs() * dm + dm * dm) * SLACK
    return m, v, dm, dv


def check_fwd_stats(what, P, m, v, dm, dv, gamma, beta, eps, scale, shift, mean, invstd, rm0=None, rv0=None, rm=None, rv=None, save_var=None):
    """The finalize: mean = (float) m; invstd = 1 / sqrtf((float) v + eps); scale = gamma invstd; shift = beta - mean scale; running
    statistics r = (1 - mom) r + mom b with the unbiased variance v n / (n - 1) (v when n = 1)."""
    gamma, beta = gamma.double(), beta.double()
    dmean = dm + U * (m.abs() + dm) * SLACK                         # + the cast to fp32
    check(mean, m, dmean, f"{what}: mean")
    inv = 1.0 / torch.sqrt(v + eps)
    # var cast (U), + eps (U), sqrtf and the division (up to 2 ulp each allowed: 4U); a relative error e of v + eps is e / 2 in invstd
    rel = (0.5 * (dv + U * (v + dv) + U * (v + dv + eps)) / (v + eps) + 4 * U) * SLACK
    check(invstd, inv, rel * inv, f"{what}: invstd")
    sc = gamma * inv
    dsc = (rel + U) * sc.abs() * SLACK
    check(scale, sc, dsc, f"{what}: scale")
    sh = beta - m * sc
    check(shift, sh, (dmean * sc.abs() + (m.abs() + dmean) * dsc + 2 * U * ((m * sc).abs() + beta.abs())) * SLACK + TINY, f"{what}: shift")
    mom = float(torch.tensor(MOM, dtype=torch.float32))
    corr = P / (P - 1) if P > 1 else 1.0
    unb, dunb = v * corr, (dv * corr + U * (v * corr + dv * corr)) * SLACK   # + the cast of the unbiased variance
    if rm is not None:
        rm0, rv0 = rm0.double(), rv0.double()
        # (1 - mom) in fp32 (U), two products and a sum (3U) of the update
        check(rm, (1 - mom) * rm0 + mom * m, (mom * dmean + 4 * U * ((1 - mom) * rm0.abs() + mom * m.abs())) * SLACK + TINY, f"{what}: running mean")
        check(rv, (1 - mom) * rv0 + mom * unb, (mom * dunb + 4 * U * ((1 - mom) * rv0.abs() + mom * unb)) * SLACK + TINY, f"{what}: running var")
    if save_var is not None:
        check(save_var, unb, dunb + TINY, f"{what}: unbiased variance")


def y_ref_check(what, x64, scale, shift, y, relu, dt):
    """y = relu?(fmaf(scale, x, shift)) from the kernel's own scale / shift: one fp32 rounding, plus the store in dt."""
    z = scale.double() * x64 + shift.double()
    r = z.clamp_min(0) if relu else z
    b = (U + (UB if dt != torch.float32 else 0.0)) * r.abs() * SLACK + TINY
    check(y.reshape(r.shape), r, b, what)


def bwd_ref(x64, g64, sc, sh, sl, mu, inv, act):
    """dz = g act'(z) with z = scale x + shift (act 3: ReLU, act 2: PReLU with slope sl, else identity), xhat = (x - mean) invstd."""
    sc, sh, mu, inv = sc.double(), sh.double(), mu.double(), inv.double()
    z = sc * x64 + sh                   # exact product of two floats; the sign is that of the kernel's fmaf
    pos = z > 0
    if act == 3:
        dz = torch.where(pos, g64, torch.zeros_like(g64))
    elif act == 2:
        dz = torch.where(pos, g64, g64 * sl.double())
    else:
        dz = g64
    xh = (x64 - mu) * inv
    return z, pos, dz, xh


def check_bwd(what, run, x64, g64, sc, sh, sl, mu, inv, act, training, dt, c1c2, draw=None, dgamma=None, dbeta=None, dslope=None, pre=None):
    """Parameter gradients (dbeta = sum dz, dgamma = sum dz xhat, dslope = sum g z [z <= 0]; added to ``pre``), the two means of the
    apply pass (0 in eval mode) and draw = scale (dz - c1 - xhat c2): the closed form of float64 autograd of act(batch_norm(x))."""
    P, C = x64.shape
    z, pos, dz, xh = bwd_ref(x64, g64, sc, sh, sl, mu, inv, act)
    S0, S1 = dz.sum(0), (dz * xh).sum(0)
    # dz: one fp32 product under PReLU (U); xhat: a subtraction and a product (2U); the fma into the run (covered by run U)
    d0 = ((run + 1) * U + FOLD) * dz.abs().sum(0) * SLACK
    d1 = ((run + 4) * U + FOLD) * (dz * xh).abs().sum(0) * SLACK
    p0 = pre[0].double() if pre is not None else 0.0
    for got, S, dS, pv, name in ((dbeta, S0, d0, p0, "dbeta"), (dgamma, S1, d1, pre[1].double() if pre is not None else 0.0, "dgamma")):
        if got is not None:
            check(got, pv + S, dS + U * (S.abs() + dS) + U * (torch.as_tensor(pv).abs() + S.abs() + dS) * SLACK + TINY, f"{what}: {name}")
    if dslope is not None:
        t = torch.where(pos, torch.zeros_like(g64), g64 * z)
        S2 = t.sum(0)
        d2 = ((run + 2) * U + FOLD) * t.abs().sum(0) * SLACK        # z and g z rounded in fp32
        pv = pre[2].double() if pre is not None else 0.0
        check(dslope, pv + S2, d2 + U * (S2.abs() + d2) + U * (torch.as_tensor(pv).abs() + S2.abs() + d2) * SLACK + TINY, f"{what}: dslope")
    c1, c2 = c1c2[:C], c1c2[C:]
    if training:
        check(c1, S0 / P, (d0 / P + U * S0.abs() / P) * SLACK + TINY, f"{what}: c1 = mean(dz)")
        check(c2, S1 / P, (d1 / P + U * S1.abs() / P) * SLACK + TINY, f"{what}: c2 = mean(dz xhat)")
    else:
        assert torch.equal(c1c2, torch.zeros_like(c1c2)), f"{what}: eval mode c1 = c2 = 0"
    if draw is None:
        return
    c1d, c2d, scd = c1.double(), c2.double(), sc.double()
    r = scd * (dz - c1d - xh * c2d)
    # from the kernel's own c1 / c2: dz (U), xhat (2U), xhat c2 (U), two subtractions (2U), the product with scale (U)
    b = 7 * U * scd.abs() * (dz.abs() + c1d.abs() + (xh * c2d).abs()) * SLACK + (UB if dt != torch.float32 else 0.0) * r.abs() * SLACK + TINY
    check(draw.reshape(r.shape), r, b, f"{what}: draw")


# ================================================================================================ 1. unet_bn: K.bn_fwd / K.bn_bwd
BN_CHANNELS = [8, 16, 32, 64, 128, 256, 512, 1024, 2048]        # every power of two chan_ok accepts


def bn_counts(C):
    """Below the 256-block cap (ragged), exactly at it, and 1.5x past it with a ragged last block."""
    cap = bn_cap(C)
    return {"below": cap // 3 + 37, "at": cap, "above": cap + cap // 2 + 13}


def run_bn(K, x, C, shape, dt, gamma, beta, *, training=True, relu=True, want_y=True, rm=None, rv=None):
    vec = nan(4, C)
    y = nan(*shape, C, dtype=dt) if want_y else None
    K.bn_fwd(nhwc(x, shape), gamma, beta, EPS_BN, MOM, rm, rv, training, vec[0], vec[1], vec[2], vec[3], y=y, relu=relu)
    return vec, y


def bn_case(K, C, P, dt, seed, ratio=None, sentinels=True):
    g = gen(seed)
    ppb, blocks = bn_plan(P, C)
    sent = sentinel_pixels(P, ppb, blocks) if sentinels else []
    x = raw_like(g, P, C, dt, ratio, sent)
    gy = grad_like(g, P, C, dt, sent)
    gamma = torch.rand(C, generator=g, device=DEV) + 0.5
    beta = torch.randn(C, generator=g, device=DEV) * 0.5
    return x, gy, gamma, beta, (ppb, blocks, sent)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", BN_CHANNELS)
@pytest.mark.parametrize("where", ["below", "at", "above"])
def test_bn_fwd_bwd_across_the_grid_cap(K, C, dt, where):
    """Statistics, scale / shift, running statistics, y and the backward (accumulating into pre-filled parameter gradients) at pixel
    counts below, at and past plan_blocks' 256-block cap, with sentinels at the block boundaries and the ragged last block."""
    P = bn_counts(C)[where]
    x, gy, gamma, beta, (ppb, blocks, sent) = bn_case(K, C, P, dt, 100 + C)
    # past the cap the grid is ceil(P / ppb) <= 256 blocks of more than 16 pixels per thread, the last one ragged
    assert (P > bn_cap(C)) == (where == "above") and (where != "at" or (blocks == 256 and P % ppb == 0)) and (where != "above" or P % ppb != 0)
    shape = (1, 1, P) if P % 7 else (7, 1, P // 7)
    rm0, rv0 = torch.randn(C, device=DEV), torch.rand(C, device=DEV) + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    vec, y = run_bn(K, x, C, shape, dt, gamma, beta, rm=rm, rv=rv)
    x64 = x.double()
    m, v, dm, dv = stats_ref(x64, RUN_BN)
    what = f"bn C={C} P={P} {dt}"
    check_fwd_stats(what, P, m, v, dm, dv, gamma, beta, EPS_BN, vec[0], vec[1], vec[2], vec[3], rm0, rv0, rm, rv)
    y_ref_check(f"{what}: y", x64, vec[0], vec[1], y, True, dt)
    pre = torch.randn(2, C, device=DEV)
    dg, db, c1c2, draw = pre[1].clone(), pre[0].clone(), nan(2 * C), nan(*shape, C, dtype=dt)
    K.bn_bwd(nhwc(x, shape), nhwc(gy, shape), vec[0], vec[1], vec[2], vec[3], dg, db, c1c2, draw, training=True, relu=True, accumulate=True)
    check_bwd(what, RUN_BN, x64, gy.double(), vec[0], vec[1], None, vec[2], vec[3], 3, True, dt, c1c2, draw, dg, db, pre=pre)


@pytest.fixture(scope="module")
def bn_shared(K):
    """One tensor past the cap (C = 64: 196,621 pixels, ragged), shared by the variant tests."""
    C = 64
    P = bn_counts(C)["above"]
    x, gy, gamma, beta, plan = bn_case(K, C, P, torch.bfloat16, 7)
    return C, P, (1, 1, P), x, gy, gamma, beta


@pytest.mark.parametrize("relu,want_y", [(False, True), (True, False)])
def test_bn_fwd_variants(K, bn_shared, relu, want_y):
    """relu=False (y = scale raw + shift, negative values kept) and y=None (statistics only: nothing else is written)."""
    C, P, shape, x, gy, gamma, beta = bn_shared
    vec, y = run_bn(K, x, C, shape, torch.bfloat16, gamma, beta, relu=relu, want_y=want_y)
    x64 = x.double()
    m, v, dm, dv = stats_ref(x64, RUN_BN)
    check_fwd_stats("bn variant", P, m, v, dm, dv, gamma, beta, EPS_BN, vec[0], vec[1], vec[2], vec[3])
    if want_y:
        y_ref_check("bn relu=False: y", x64, vec[0], vec[1], y, relu, torch.bfloat16)
        assert (y < 0).any()


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("accumulate,params", [(True, True), (False, True), (True, False)])
def test_bn_bwd_variants(K, bn_shared, training, accumulate, params):
    """Training and eval mode (c1 = c2 = 0), accumulate on and off (pre-filled parameter gradients added to or overwritten),
    dgamma = dbeta = None, relu off, and the in-place call of arch/unet.py (draw is g): bit for bit the out-of-place result."""
    C, P, shape, x, gy, gamma, beta = bn_shared
    dt = torch.bfloat16
    rm, rv = torch.randn(C, device=DEV) * 0.1, torch.rand(C, device=DEV) + 0.5
    vec, _ = run_bn(K, x, C, shape, dt, gamma, beta, training=training, want_y=False, rm=rm.clone(), rv=rv.clone())
    x64, g64 = x.double(), gy.double()
    for relu in (True, False):
        pre = torch.randn(2, C, device=DEV)
        dg, db = (pre[1].clone(), pre[0].clone()) if params else (None, None)
        c1c2, draw = nan(2 * C), nan(*shape, C, dtype=dt)
        K.bn_bwd(nhwc(x, shape), nhwc(gy, shape), vec[0], vec[1], vec[2], vec[3], dg, db, c1c2, draw, training=training, relu=relu,
                 accumulate=accumulate)
        check_bwd(f"bn bwd training={training} accumulate={accumulate} relu={relu}", RUN_BN, x64, g64, vec[0], vec[1], None, vec[2], vec[3],
                  3 if relu else 0, training, dt, c1c2, draw, dg, db, pre=pre if accumulate else None)
        if relu and params:
            g2 = gy.clone()
            pre2 = torch.randn(2, C, device=DEV)
            dg2, db2, cc2 = pre2[1].clone(), pre2[0].clone(), nan(2 * C)
            K.bn_bwd(nhwc(x, shape), nhwc(g2, shape), vec[0], vec[1], vec[2], vec[3], dg2, db2, cc2, nhwc(g2, shape), training=training,
                     relu=True, accumulate=accumulate)
            assert torch.equal(g2.view_as(draw), draw) and torch.equal(cc2, c1c2), "in-place bn_bwd (draw is g)"


def test_bn_eval_fwd_reads_running_statistics_only(K, bn_shared):
    """Eval mode: mean / invstd from the running statistics, which stay untouched; no reduction is launched (the workspace keeps
    its bytes)."""
    C, P, shape, x, gy, gamma, beta = bn_shared
    rm, rv = torch.randn(C, device=DEV), torch.rand(C, device=DEV) + 0.5
    rm0, rv0 = rm.clone(), rv.clone()
    from dct_amd import _lib
    ws = K._enet_ws(x.device, _lib.load().dct_bn_workspace_bytes(C))
    ws.fill_(0x5A)
    ws0 = ws.clone()
    vec, y = run_bn(K, x, C, shape, torch.bfloat16, gamma, beta, training=False, rm=rm, rv=rv)
    torch.cuda.synchronize()
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0) and torch.equal(ws, ws0)
    assert torch.equal(vec[2], rm0)
    inv = 1.0 / torch.sqrt(rv0.double() + EPS_BN)
    check(vec[3], inv, 6 * U * inv, "eval invstd")          # + eps, sqrtf, division: one rounding, 2 ulp, 2 ulp
    y_ref_check("eval y", x.double(), vec[0], vec[1], y, True, torch.bfloat16)


@pytest.mark.parametrize("P", [1, 5])
def test_bn_tiny_batches(K, P):
    """count = 1: variance 0 and the running variance takes the biased value (no n / (n - 1) at n = 1); count = 5: the unbiased
    correction is 5/4."""
    C = 128
    g = gen(11)
    x = raw_like(g, P, C, torch.float32)
    gamma, beta = torch.rand(C, generator=g, device=DEV) + 0.5, torch.randn(C, generator=g, device=DEV)
    rm0, rv0 = torch.randn(C, device=DEV), torch.rand(C, device=DEV) + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    vec, y = run_bn(K, x, C, (1, 1, P), torch.float32, gamma, beta, rm=rm, rv=rv)
    m, v, dm, dv = stats_ref(x.double(), RUN_BN)
    check_fwd_stats(f"bn P={P}", P, m, v, dm, dv, gamma, beta, EPS_BN, vec[0], vec[1], vec[2], vec[3], rm0, rv0, rm, rv)
    y_ref_check(f"bn P={P}: y", x.double(), vec[0], vec[1], y, True, torch.float32)


def test_bn_strided_channel_slices(K):
    """vec8_ok accepts strided NHWC views: raw, y, g and draw as channel slices of wider buffers; the channels outside the slices keep
    their bits."""
    C, Cw, lo = 128, 384, 64
    B, H, W = 3, 97, 89                   # 25,899 pixels: past the C = 128 cap (16,384)
    P = B * H * W
    g = gen(21)
    dt = torch.bfloat16
    wide = torch.randn(B, H, W, Cw, generator=g, device=DEV).to(dt)
    ppb, blocks = bn_plan(P, C)
    xs = raw_like(g, P, C, dt, sentinels=sentinel_pixels(P, ppb, blocks))
    wide[..., lo:lo + C] = xs.view(B, H, W, C)
    gw = torch.randn(B, H, W, Cw, generator=g, device=DEV).to(dt)
    yw, dw = torch.randn_like(gw), torch.randn_like(gw)
    keep = [t.clone() for t in (wide, gw, yw, dw)]
    raw, gv, yv, dv_ = (t[..., lo:lo + C] for t in (wide, gw, yw, dw))
    gamma, beta = torch.rand(C, generator=g, device=DEV) + 0.5, torch.randn(C, generator=g, device=DEV)
    vec = nan(4, C)
    K.bn_fwd(raw, gamma, beta, EPS_BN, MOM, None, None, True, vec[0], vec[1], vec[2], vec[3], y=yv, relu=True)
    c1c2 = nan(2 * C)
    K.bn_bwd(raw, gv, vec[0], vec[1], vec[2], vec[3], None, None, c1c2, dv_, training=True, relu=True)
    x64 = raw.reshape(P, C).double()
    m, v, dm, dv = stats_ref(x64, RUN_BN)
    check_fwd_stats("bn view", P, m, v, dm, dv, gamma, beta, EPS_BN, vec[0], vec[1], vec[2], vec[3])
    y_ref_check("bn view: y", x64, vec[0], vec[1], yv, True, dt)
    check_bwd("bn view", RUN_BN, x64, gv.reshape(P, C).double(), vec[0], vec[1], None, vec[2], vec[3], 3, True, dt, c1c2, dv_)
    for t, t0, name in zip((wide, gw, yw, dw), keep, ("raw", "g", "y", "draw")):
        outside = torch.cat((t[..., :lo], t[..., lo + C:]), -1).view(torch.int16)
        assert torch.equal(outside, torch.cat((t0[..., :lo], t0[..., lo + C:]), -1).view(torch.int16)), f"{name}: channels outside the slice"
    assert torch.equal(wide, keep[0]) and torch.equal(gw, keep[1])


def test_bn_refuses_unsupported_layouts(K):
    """Channel counts chan_ok / vec8_ok reject and a misaligned base raise instead of computing; the outputs stay as they were."""
    g = gen(31)
    for C, off, Cw in ((24, 0, 24), (4, 0, 4), (64, 4, 72)):
        buf = torch.randn(2, 5, 7, Cw, generator=g, device=DEV).to(torch.bfloat16)
        raw = buf[..., off:off + C]
        vec = nan(4, C)
        y = torch.zeros(2, 5, 7, C, dtype=torch.bfloat16, device=DEV)
        with pytest.raises(RuntimeError):
            K.bn_fwd(raw, torch.ones(C, device=DEV), torch.zeros(C, device=DEV), EPS_BN, MOM, None, None, True,
                     vec[0], vec[1], vec[2], vec[3], y=y)
        with pytest.raises(RuntimeError):
            K.bn_bwd(raw, raw, torch.ones(C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), torch.ones(C, device=DEV),
                     None, None, nan(2 * C), y, training=True)
        torch.cuda.synchronize()
        assert torch.isnan(vec).all() and not y.any(), (C, off)


@pytest.fixture(scope="module")
def unet_bn_shapes(K):
    """The raw conv outputs unet_bn's plan hands K.bn_fwd at 256 x 256 with cfg2's batch (bench.py: 8 labelled and 8 unlabelled
    slices, one forward pass each: BatchNorm couples a pass's samples), read from one training forward of the model."""
    from dct_amd.arch import get_arch
    net = get_arch("unet_bn", {"num_classes": 4, "compute_dtype": torch.bfloat16, "dropout_p": 0.0}).to(DEV).train()
    seen = []
    orig = K.bn_fwd

    def record(raw, *a, **kw):
        seen.append((tuple(raw.shape), raw.dtype))
        return orig(raw, *a, **kw)
    K.bn_fwd = record
    try:
        with torch.no_grad():
            net(torch.rand(8, 1, 256, 256, generator=gen(1), device=DEV))
    finally:
        K.bn_fwd = orig
    torch.cuda.synchronize()
    assert len(seen) == 13, seen          # 4 encoder blocks + enc1 + 2 centre + 2 x 3 decoder convolutions feed a BatchNorm
    return sorted(set(seen))


def test_bn_at_unet_bn_plan_shapes(K, unet_bn_shapes):
    """Forward and backward at every BatchNorm shape of unet_bn at 256^2 (bf16), the full-resolution ones past the grid cap."""
    for k, (shape, dt) in enumerate(unet_bn_shapes):
        B, H, W, C = shape
        P = B * H * W
        x, gy, gamma, beta, (ppb, blocks, _) = bn_case(K, C, P, dt, 200 + k)
        vec, y = run_bn(K, x, C, (B, H, W), dt, gamma, beta)
        x64 = x.double()
        m, v, dm, dv = stats_ref(x64, RUN_BN)
        what = f"unet_bn {shape} ({blocks} blocks of {ppb})"
        check_fwd_stats(what, P, m, v, dm, dv, gamma, beta, EPS_BN, vec[0], vec[1], vec[2], vec[3])
        y_ref_check(f"{what}: y", x64, vec[0], vec[1], y, True, dt)
        c1c2, draw = nan(2 * C), nan(B, H, W, C, dtype=dt)
        dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        K.bn_bwd(nhwc(x, (B, H, W)), nhwc(gy, (B, H, W)), vec[0], vec[1], vec[2], vec[3], dg, db, c1c2, draw, training=True, relu=True,
                 accumulate=False)
        check_bwd(what, RUN_BN, x64, gy.double(), vec[0], vec[1], None, vec[2], vec[3], 3, True, dt, c1c2, draw, dg, db)
    # at 8 slices of 256^2 the two 64-channel full-resolution BatchNorms (enc1, dec1) are past the cap; the narrower-image, wider-channel
    # layers stay below it
    assert sum(s[0] * s[1] * s[2] > bn_cap(s[3]) for s, _ in unet_bn_shapes) >= 2, unet_bn_shapes


# ================================================================================================ 2. Enet BatchNorm (csrc/enet.hip)
ENET_CHANNELS = [3, 13, 24, 16, 32, 64, 128]     # 16 ... 128: ReduceVecK; 3, 13, 24: ReduceK


def make_tf(K, g, C, mode, fwd):
    sl = torch.rand(C, generator=g, device=DEV) * 0.5
    return K.Tf(fwd[0], fwd[1], sl if mode == 2 else None, mode), sl


def run_enet_fwd(K, raw, gamma, beta, training=True, **kw):
    C = raw.shape[3]
    vec = nan(5, C)
    K.enet_bn_fwd_stats(raw, gamma, beta, EPS_ENET, MOM, None, None, training, vec[0], vec[1], vec[2], vec[3], save_var=vec[4], **kw)
    return vec


def enet_bwd_all(K, raw, gd, mask, tf, vec, C, dt, pre, act):
    """enet_bn_bwd and its split form (sums, then apply) on the same inputs; the split must give the same bits."""
    outs = []
    for split in (False, True):
        dg, db, ds = pre[1].clone(), pre[0].clone(), pre[2].clone()
        c1c2, draw = nan(2 * C), nan(*raw.shape[:3], C, dtype=dt)
        args = (raw, gd, mask, tf, vec[2], vec[3], dg, db, ds if act == 2 else None, c1c2)
        if split:
            K.enet_bn_bwd_sums(*args)
            K.enet_bn_bwd_apply(raw, gd, mask, tf, vec[2], vec[3], c1c2, draw)
        else:
            K.enet_bn_bwd(*args, draw)
        outs.append((dg, db, ds, c1c2, draw))
    for a, b, name in zip(outs[0], outs[1], ("dgamma", "dbeta", "dslope", "c1c2", "draw")):
        assert torch.equal(a, b), f"split backward: {name}"
    return outs[0]


def enet_case(K, shape, C, dt, act, seed, use_mask, ratio=None):
    g = gen(seed)
    P = shape[0] * shape[1] * shape[2]
    ppb, blocks = enet_plan(P, C)
    sent = sentinel_pixels(P, ppb, blocks)
    raw = raw_like(g, P, C, torch.float32, ratio, sent)          # Enet's raw conv outputs are fp32 in every mode
    gy = grad_like(g, P, C, dt, sent)
    mask = torch.randn(P, C, generator=g, device=DEV).to(dt) if use_mask else None
    if mask is not None:
        mask[sent] = 1.0                                         # the sentinels' gradients pass the gate
    gamma, beta = torch.rand(C, generator=g, device=DEV) + 0.5, torch.randn(C, generator=g, device=DEV) * 0.5
    vec = run_enet_fwd(K, nhwc(raw, shape), gamma, beta)
    x64 = raw.double()
    m, v, dm, dv = stats_ref(x64, RUN_ENET)
    what = f"enet {shape} C={C} act={act} {dt} mask={use_mask} ({blocks} blocks of {ppb})"
    check_fwd_stats(what, P, m, v, dm, dv, gamma, beta, EPS_ENET, vec[0], vec[1], vec[2], vec[3], save_var=vec[4])
    tf, sl = make_tf(K, g, C, {0: 1, 2: 2, 3: 3}[act], vec)
    pre = torch.randn(3, C, generator=g, device=DEV)
    gd, md = nhwc(gy, shape), (nhwc(mask, shape) if mask is not None else None)
    dg, db, ds, c1c2, draw = enet_bwd_all(K, nhwc(raw, shape), gd, md, tf, vec, C, dt, pre, act)
    g64 = gy.double() if mask is None else torch.where(mask > 0, gy, torch.zeros_like(gy)).double()
    check_bwd(what, RUN_ENET, x64, g64, vec[0], vec[1], sl, vec[2], vec[3], act, True, dt, c1c2, draw, dg, db,
              ds if act == 2 else None, pre=pre)
    return P > enet_cap(C)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("act", [0, 2, 3])
@pytest.mark.parametrize("C", ENET_CHANNELS)
def test_enet_bn_past_the_grid_cap(K, C, act, dt):
    """enet_bn_fwd_stats / enet_bn_bwd (and the split sums + apply, bit for bit) at twice red_plan's cap plus a ragged tail, every
    activation mode, with and without the gradient's ReLU gate; the finalize adds to pre-filled dgamma / dbeta / dslope."""
    P = 2 * enet_cap(C) + 29
    shape = (1, 1, P)
    for use_mask in (False, True):
        assert enet_case(K, shape, C, dt, act, 300 + C + act, use_mask)


@pytest.fixture(scope="module")
def enet_shapes(K):
    """Raw shapes the Enet plan hands its BatchNorms at 256^2 with cfg4's adversarial batch (8 + 8) and 320^2 with cfg5's (4 + 16),
    read from one training forward each."""
    from dct_amd.arch import get_arch
    seen = []
    orig = K.enet_bn_fwd_stats

    def record(raw, *a, **kw):
        seen.append(tuple(raw.shape))
        return orig(raw, *a, **kw)
    K.enet_bn_fwd_stats = record
    try:
        for B, H in ((16, 256), (20, 320)):
            net = get_arch("enet", {"num_classes": 2, "compute_dtype": torch.bfloat16}).to(DEV).train()
            with torch.no_grad():
                net(torch.rand(B, 1, H, H, generator=gen(2), device=DEV))
    finally:
        K.enet_bn_fwd_stats = orig
    torch.cuda.synchronize()
    assert len(seen) >= 2 * 80, len(seen)
    return sorted(set(seen))


def test_enet_bn_at_plan_shapes(K, enet_shapes):
    """Every distinct BatchNorm shape of Enet at 256^2 / 320^2 (bf16 gradients, activation modes taken in turn, gated half the time)."""
    capped = 0
    for k, shape in enumerate(enet_shapes):
        act = (2, 3, 0)[k % 3]
        capped += enet_case(K, shape[:3], shape[3], torch.bfloat16, act, 400 + k, use_mask=k % 2 == 0)
    assert capped > len(enet_shapes) // 2, (capped, enet_shapes)


# ------------------------------------------------------------------------------------------------ fused statistics rows
def fold_counts(C):
    """Tile counts for fold_partials (1024 threads: NP = 1024 / next_pow2(C) partial sums per channel, 8 rows per unrolled trip):
    below 8 NP, just above one and two multiples of 8 NP (the remainder loop runs after the unrolled one), and the model's cap
    (arch/enet.py: DCT_ENET_STATS_TILES = 2560)."""
    np_ = 1024 // (1 << (C - 1).bit_length())
    return [5 * np_ + 3, 8 * np_ + 1, 16 * np_ + 5, 2560]


def conv_case(g, T, C, cin=16):
    P = 32 * T - 7                                   # the last tile ragged
    x = torch.randn(1, 1, P, cin, generator=g, device=DEV).to(torch.bfloat16)
    w = (torch.randn(C, 1, 1, cin, generator=g, device=DEV) / math.sqrt(cin)).contiguous()
    bias = torch.randn(C, generator=g, device=DEV)
    return P, x, w, bias


@pytest.mark.parametrize("C", [16, 64, 128])
def test_enet_fused_statistics_rows(K, C):
    """enet_conv_stats -> enet_bn_fwd_stats(partial_rows) and enet_conv_bnbwd_stats -> enet_bn_bwd(partial_rows) at tile counts that
    run fold_partials' unrolled loop, its remainder loop and the model's 2,560-tile cap; the folded statistics against float64 sums
    over the stored output tensor (what the consumer reads).  One tile more than the scratch holds: 0 rows, nothing written."""
    g = gen(500 + C)
    kw = dict(R=1, S=1, compute=torch.bfloat16)
    for T in fold_counts(C):
        P, x, w, bias = conv_case(g, T, C)
        stats = nan(T * C * 3, dtype=torch.float64)
        y = nan(1, 1, P, C)
        rows = K.enet_conv_stats(x, w, bias, None, y, stats, ws=(16, 16, 1), **kw)
        assert rows == T
        y2 = nan(1, 1, P, C)
        K.enet_conv(x, w, bias, None, y2, ws=(16, 16, 1), **kw)
        assert torch.equal(y, y2)
        y64 = y.reshape(P, C).double()
        st = stats.view(T, C, 3)
        k = RUN_ENET * U * SLACK
        check(st[:, :, 0].sum(0), y64.sum(0), k * y64.abs().sum(0), f"T={T}: rows sum")
        check(st[:, :, 1].sum(0), (y64 * y64).sum(0), k * (y64 * y64).sum(0), f"T={T}: rows sum of squares")
        assert (st[:, :, 2] == 0).all()
        gamma, beta = torch.rand(C, generator=g, device=DEV) + 0.5, torch.randn(C, generator=g, device=DEV)
        vec = run_enet_fwd(K, y, gamma, beta, partial=stats, partial_rows=rows)
        m, v, dm, dv = stats_ref(y64, RUN_ENET)
        what = f"fused fwd C={C} T={T}"
        check_fwd_stats(what, P, m, v, dm, dv, gamma, beta, EPS_ENET, vec[0], vec[1], vec[2], vec[3], save_var=vec[4])
        vsep = run_enet_fwd(K, y, gamma, beta)          # the separate reduction over the same tensor meets the same bounds
        check_fwd_stats(f"{what}, separate reduction", P, m, v, dm, dv, gamma, beta, EPS_ENET, vsep[0], vsep[1], vsep[2], vsep[3], save_var=vsep[4])
        # backward: the data-gradient convolution C -> 16 transposed, whose output g is this layer's activation gradient
        tf, sl = make_tf(K, g, C, 2, vec)
        gy = torch.randn(1, 1, P, 16, generator=g, device=DEV).to(torch.bfloat16)
        wd = (torch.randn(16, 1, 1, C, generator=g, device=DEV) / 4).contiguous()      # forward conv C -> 16, as K-major [16][1][1][C]
        dkw = dict(transposed=True, ws=(1, C, C), **kw)
        stats.fill_(float("nan"))
        gd = nan(1, 1, P, C, dtype=torch.bfloat16)
        rows = K.enet_conv_bnbwd_stats(gy, wd, gd, stats, y, tf, vec[2], vec[3], **dkw)
        assert rows == T and torch.isfinite(stats).all()
        gd2 = nan(1, 1, P, C, dtype=torch.bfloat16)
        K.enet_conv(gy, wd, None, None, gd2, **dkw)
        assert torch.equal(gd, gd2)
        pre = torch.randn(3, C, generator=g, device=DEV)
        dg, db, ds, c1c2, draw = pre[1].clone(), pre[0].clone(), pre[2].clone(), nan(2 * C), nan(1, 1, P, C, dtype=torch.bfloat16)
        K.enet_bn_bwd(y, gd, None, tf, vec[2], vec[3], dg, db, ds, c1c2, draw, partial=stats, partial_rows=rows)
        check_bwd(f"fused bwd C={C} T={T}", RUN_ENET, y64, gd.reshape(P, C).double(), vec[0], vec[1], sl, vec[2], vec[3], 2, True,
                  torch.bfloat16, c1c2, draw, dg, db, ds, pre=pre)
    # one tile over the scratch: no rows, the scratch untouched, y still written
    T = 2561
    P, x, w, bias = conv_case(g, T, C)
    stats = nan((T - 1) * C * 3, dtype=torch.float64)
    y = nan(1, 1, P, C)
    assert K.enet_conv_stats(x, w, bias, None, y, stats, ws=(16, 16, 1), **kw) == 0
    torch.cuda.synchronize()
    assert torch.isnan(stats).all() and torch.isfinite(y).all()


@pytest.mark.parametrize("k,act,use_mask", [(1, 2, True), (1, 3, False), (3, 2, False)])
def test_enet_normalise_on_load_past_the_cap(K, k, act, use_mask):
    """enet_conv_bwd_in (the BatchNorm backward applied while the data-gradient convolution loads its input) equals enet_conv on the
    draw enet_bn_bwd_apply stores, bit for bit, at 4 x 67 x 61 pixels (past red_plan's C = 64 cap of 8,192)."""
    g = gen(600 + k + act)
    C, Cx, shape = 64, 16, (4, 67, 61)
    P = shape[0] * shape[1] * shape[2]
    raw = raw_like(g, P, C, torch.float32).view(*shape, C)
    gamma, beta = torch.rand(C, generator=g, device=DEV) + 0.5, torch.randn(C, generator=g, device=DEV)
    vec = run_enet_fwd(K, raw, gamma, beta)
    tf, _ = make_tf(K, g, C, act, vec)
    gy = torch.randn(*shape, C, generator=g, device=DEV).to(torch.bfloat16)
    mask = torch.randn(*shape, C, generator=g, device=DEV).to(torch.bfloat16) if use_mask else None
    c1c2 = nan(2 * C)
    K.enet_bn_bwd_sums(raw, gy, mask, tf, vec[2], vec[3], None, None, None, c1c2)
    draw = nan(*shape, C, dtype=torch.bfloat16)
    K.enet_bn_bwd_apply(raw, gy, mask, tf, vec[2], vec[3], c1c2, draw)
    w = (torch.randn(C, k, k, Cx, generator=g, device=DEV) / math.sqrt(C * k * k)).contiguous()   # forward conv Cx -> C
    kw = dict(R=k, S=k, pad_h=k // 2, pad_w=k // 2, transposed=True, ws=(1, Cx, k * k * Cx), compute=torch.bfloat16)
    y1, y2 = nan(*shape, Cx, dtype=torch.bfloat16), nan(*shape, Cx, dtype=torch.bfloat16)
    K.enet_conv(draw, w, None, None, y1, **kw)
    rows = K.enet_conv_bwd_in(raw, w, tf, gy, mask, vec[2], vec[3], c1c2, y2, **kw)
    assert rows == 0
    assert torch.equal(y1, y2) and torch.isfinite(y1).all()


# ================================================================================================ 3. large mean relative to spread
@pytest.mark.parametrize("ratio", [10.0, 30.0])
def test_one_pass_variance_with_large_mean(K, ratio):
    """|mean| / std = ratio in every channel (raw conv outputs with a bias) at training-scale pixel counts: bn.hip (C = 64, fp32 and
    bf16), both Enet reductions (C = 16 vector, 13 scalar) and the MFMA epilogue's rows (C = 64).  The one-pass variance is held to
    the bound above, whose cancellation term 2 |m| dm + dm_2 grows with ratio^2; the two-pass float64 variance is the reference."""
    g = gen(700 + int(ratio))
    for dt in (torch.float32, torch.bfloat16):
        C, P = 64, 8 * 256 * 256
        x = raw_like(g, P, C, dt, ratio)
        gamma, beta = torch.rand(C, generator=g, device=DEV) + 0.5, torch.randn(C, generator=g, device=DEV)
        vec, y = run_bn(K, x, C, (8, 256, 256), dt, gamma, beta)
        m, v, dm, dv = stats_ref(x.double(), RUN_BN)
        check_fwd_stats(f"bn ratio={ratio} {dt}", P, m, v, dm, dv, gamma, beta, EPS_BN, vec[0], vec[1], vec[2], vec[3])
        vk = 1.0 / vec[3].double() ** 2 - EPS_BN             # the variance the kernel used, to the precision of invstd (~1e-7)
        print(f"bn ratio={ratio} {dt}: max relative variance error {((vk - v).abs() / v).max().item():.2e}, bound {(dv / v).min().item():.2e}")
    for C in (16, 13):
        P = 20 * 160 * 160
        x = raw_like(g, P, C, torch.float32, ratio)
        gamma, beta = torch.rand(C, generator=g, device=DEV) + 0.5, torch.randn(C, generator=g, device=DEV)
        vec = run_enet_fwd(K, x.view(20, 160, 160, C), gamma, beta)
        m, v, dm, dv = stats_ref(x.double(), RUN_ENET)
        check_fwd_stats(f"enet ratio={ratio} C={C}", P, m, v, dm, dv, gamma, beta, EPS_ENET, vec[0], vec[1], vec[2], vec[3], save_var=vec[4])
        print(f"enet ratio={ratio} C={C}: max relative variance error {((vec[4].double() - v * P / (P - 1)).abs() / v).max().item():.2e}, "
              f"bound {(dv / v).min().item():.2e}")
    C, T = 64, 2560
    P, x, w, bias = conv_case(g, T, C)
    y0 = nan(1, 1, P, C)
    K.enet_conv(x, w, torch.zeros(C, device=DEV), None, y0, R=1, S=1, ws=(16, 16, 1), compute=torch.bfloat16)
    sd = y0.reshape(P, C).double().std(0).float()
    bias = ratio * sd * torch.where(torch.rand(C, generator=g, device=DEV) < 0.5, -1.0, 1.0)
    stats, y = nan(T * C * 3, dtype=torch.float64), nan(1, 1, P, C)
    rows = K.enet_conv_stats(x, w, bias, None, y, stats, R=1, S=1, ws=(16, 16, 1), compute=torch.bfloat16)
    assert rows == T
    gamma, beta = torch.rand(C, generator=g, device=DEV) + 0.5, torch.randn(C, generator=g, device=DEV)
    vec = run_enet_fwd(K, y, gamma, beta, partial=stats, partial_rows=rows)
    m, v, dm, dv = stats_ref(y.reshape(P, C).double(), RUN_ENET)
    assert (m.abs() / v.sqrt()).min() > 0.9 * ratio
    check_fwd_stats(f"epilogue rows ratio={ratio}", P, m, v, dm, dv, gamma, beta, EPS_ENET, vec[0], vec[1], vec[2], vec[3], save_var=vec[4])
