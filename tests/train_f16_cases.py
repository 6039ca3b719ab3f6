"""Float64 references and case tables of the fp16 training kernels (train_f16.hip, wgrad_mfma_f16.hip, the data-gradient
banks through ds_conv_fwd_f16), shared by the emulator suite (test_emul_train_f16.py) and the device suite
(test_gpu_train_f16_kernels.py).  A plain helper module: host arrays in, host arrays out, no fixtures.

Every reference sees the SAME fp16-rounded operands as the kernel (callers round with `r16` first) and computes in
float64.  Small cases go through the numpy oracle (deepspeaker_oracle); the convolution backward also has a torch float64
form, chunked over the batch, because the oracle's im2col is too slow (and too large) at real layer sizes.

Layouts: the kernels' own.  Element-wise / BatchNorm tensors are [G * n_pix, C] (NHWC with the pixels flattened, member m
owns rows [m * n_pix, (m + 1) * n_pix)); convolution tensors are NCHW on the reference side as the oracle takes them."""
import numpy as np
import torch

import deepspeaker_oracle as O

CLIP_MAX = 20.0
TF_PIX_BUDGET = 16384          # ds_bn_f16_partial_rows: ppb = max(8, 16384 / C) pixels per row, at most TF_MAX_ROWS rows
TF_MAX_ROWS = 768
TF_FOLD_R = 128                # rows stepped by the fold's row lanes
TF_GRID_CAP = 8192             # workgroups of an element-wise launch; above 8192 * 256 vectors of 8 halfs: grid-stride loop
REF_CHUNK_BYTES = 1 << 30      # no float64 temporary of a chunked reference exceeds about this


def r16(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def expected_rows(n_pix, c):
    """what ds_bn_f16_partial_rows must return (tf_rows in train_f16.hip), and the pixels per row the launches then use"""
    ppb = max(TF_PIX_BUDGET // c, 8)
    rows = min((n_pix + ppb - 1) // ppb, TF_MAX_ROWS)
    return rows, (n_pix + rows - 1) // rows


def empty_trailing_rows(n_pix, c):
    """partial rows past the last pixel: they must hold zeros, not stale sums"""
    rows, ppb = expected_rows(n_pix, c)
    return rows - (n_pix + ppb - 1) // ppb


def _threads():
    if torch.get_num_threads() != 16:
        torch.set_num_threads(16)


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm statistics
# ---------------------------------------------------------------------------------------------------------------------
def bn_member_stats(z, G):
    """z [G * n_pix, C] (fp16 values) -> float64 (mean [G, C], biased var [G, C]); two-pass, chunked"""
    _threads()
    z = np.asarray(z)
    n_pix, c = z.shape[0] // G, z.shape[1]
    mean, var = np.empty((G, c)), np.empty((G, c))
    step = max(1, REF_CHUNK_BYTES // (8 * c))
    for m in range(G):
        zm = torch.from_numpy(z[m * n_pix:(m + 1) * n_pix])
        s = torch.zeros(c, dtype=torch.float64)
        for p in range(0, n_pix, step):
            s += zm[p:p + step].double().sum(0)
        mu = s / n_pix
        q = torch.zeros(c, dtype=torch.float64)
        for p in range(0, n_pix, step):
            q += ((zm[p:p + step].double() - mu) ** 2).sum(0)
        mean[m], var[m] = mu.numpy(), (q / n_pix).numpy()
    return mean, var


def bn_tables_ref(mean, var, gamma, beta, eps):
    """float64 (invstd, scale, shift) [G, C] of per-member batch statistics"""
    invstd = 1.0 / np.sqrt(var + eps)
    scale = gamma.astype(np.float64)[None] * invstd
    return invstd, scale, beta.astype(np.float64)[None] - mean * scale


def bn_running_ref(mean, var, n_pix, rm, rv, momentum):
    """the G momentum updates of the running statistics, members in call order (float64)"""
    erm, erv = rm.astype(np.float64), rv.astype(np.float64)
    for m in range(mean.shape[0]):
        erm = (1 - momentum) * erm + momentum * mean[m]
        erv = (1 - momentum) * erv + momentum * var[m] * n_pix / max(n_pix - 1, 1)
    return erm, erv


def partition_sums_f32(v1, v2, c):
    """float32 tensors v1, v2 [n_pix, C] of one member -> float64 (sum v1, sum v2) [C] in the partition the reductions
    document: rows of ppb pixels (expected_rows), inside a row a thread ("slot", 256 / (C / 8) of them) adds every
    slots-th pixel in order in float32, the slots are added in order in float32 (block_fold), the rows in float64."""
    n_pix = v1.shape[0]
    rows, ppb = expected_rows(n_pix, c)
    slots = 256 // (c // 8)
    steps = (ppb + slots - 1) // slots
    out = []
    for v in (v1, v2):
        t = torch.zeros((rows, steps * slots, c), dtype=torch.float32)
        full = n_pix // ppb                                 # rows that hold ppb pixels
        t[:full, :ppb] = v[:full * ppb].view(full, ppb, c)
        if full * ppb < n_pix:
            t[full, :n_pix - full * ppb] = v[full * ppb:]
        t = t.view(rows, steps, slots, c)
        acc = torch.zeros((rows, slots, c), dtype=torch.float32)
        for k in range(steps):
            acc += t[:, k]
        row = torch.zeros((rows, c), dtype=torch.float32)
        for k in range(slots):
            row += acc[:, k]
        out.append(row.double().sum(0))
    return out


def bn_stats_f32_restatement(z, G, eps):
    """The statistics as the kernel documents them, restated on the CPU: float32 partial sums of z and z^2
    (partition_sums_f32), var = E[z^2] - mean^2 in float64.  Its distance from bn_member_stats is the error ANY float32
    implementation of this partition carries: the yardstick of the large-reduction bars (never the kernel's own
    output).  -> float64 (mean, var, invstd) [G, C]"""
    _threads()
    z = np.asarray(z)
    n_pix, c = z.shape[0] // G, z.shape[1]
    mean, var, invstd = np.empty((G, c)), np.empty((G, c)), np.empty((G, c))
    for m in range(G):
        zm = torch.from_numpy(z[m * n_pix:(m + 1) * n_pix]).float()
        t1, t2 = partition_sums_f32(zm, zm * zm, c)
        mu = t1 / n_pix
        v = (t2 / n_pix - mu * mu).clamp_min(0.0)
        mean[m], var[m], invstd[m] = mu.numpy(), v.numpy(), (1.0 / torch.sqrt(v + eps)).numpy()
    return mean, var, invstd


def bn_bwd_sums_f32_restatement(z, gy, mean_t, invstd_t, G):
    """dgamma / dbeta (loss-scaled units, members added as float32 values like the kernel's fold) from float32 partial sums
    of gy and gy * xhat in the kernel's partition: the yardstick for the large backward reductions"""
    _threads()
    z, gy = np.asarray(z), np.asarray(gy)
    n_pix, c = z.shape[0] // G, z.shape[1]
    gg, gb = np.zeros(c), np.zeros(c)
    for m in range(G):
        sl = slice(m * n_pix, (m + 1) * n_pix)
        zm, gm = torch.from_numpy(z[sl]).float(), torch.from_numpy(gy[sl]).float()
        mu, inv = torch.from_numpy(np.asarray(mean_t[m], np.float32)), torch.from_numpy(np.asarray(invstd_t[m], np.float32))
        t1, t2 = partition_sums_f32(gm, gm * ((zm - mu) * inv), c)
        gb += t1.float().double().numpy()
        gg += t2.float().double().numpy()
    return gg, gb


def bn_apply_errors(got, z, scale_t, shift_t, res, G, clip):
    """(max |got - y|, max |y|) for float64 y = clip(z * scale[m] + shift[m] (+ res)) over [G * n_pix, C], with the tables
    the kernel was given; chunked, every element compared"""
    _threads()
    z, got = np.asarray(z), np.asarray(got)
    n_pix = z.shape[0] // G
    step = max(1, REF_CHUNK_BYTES // (8 * 4 * z.shape[1]))
    worst, top = 0.0, 0.0
    for m in range(G):
        sc, sh = torch.from_numpy(np.asarray(scale_t[m], np.float64)), torch.from_numpy(np.asarray(shift_t[m], np.float64))
        for p in range(m * n_pix, (m + 1) * n_pix, step):
            q = min(p + step, (m + 1) * n_pix)
            y = torch.from_numpy(z[p:q]).double() * sc + sh
            if res is not None:
                y += torch.from_numpy(np.asarray(res[p:q])).double()
            if clip:
                y.clamp_(0.0, CLIP_MAX)
            d = (torch.from_numpy(got[p:q]).double() - y).abs()
            d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)     # a NaN left in the output fails
            worst, top = max(worst, float(d.max())), max(top, float(y.abs().max()))
    return worst, top


def act_from_z(z, scale_t, shift_t, G):
    """The activation ds_bn_apply_group_f16 stores for clip(z * scale[m] + shift[m]) with no residual, as fp16 [G * n_pix, C],
    recomputed on the host: fp16 z times f32 scale is exact in float64, so float64 mul + add rounded to f32 is the fma's
    single rounding (but for sums that land within 2^-29 ulp of an f32 midpoint), then clip and the fp16 rounding."""
    z = np.asarray(z)
    n_pix = z.shape[0] // G
    out = np.empty(z.shape, np.float16)
    for m in range(G):
        sl = slice(m * n_pix, (m + 1) * n_pix)
        y = z[sl].astype(np.float64) * scale_t[m].astype(np.float64) + shift_t[m].astype(np.float64)
        out[sl] = np.clip(y.astype(np.float32), np.float32(0), np.float32(CLIP_MAX)).astype(np.float16)
    return out


def bn_apply_bar(top, out_f32):
    """the emulator test's bar: f32 output to 1e-5 absolute, fp16 output to an eighth of a percent of the largest value"""
    return 1e-5 if out_f32 else 1e-2 * max(1.0, top) * 2 ** -3


def tol_err(got, ref, atol=0.0):
    """the smallest rtol with which np.testing.assert_allclose(got, ref, rtol, atol) passes"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.clip(np.abs(got - ref) - atol, 0.0, None) / np.maximum(np.abs(ref), 1e-300)).max())


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm + clipped-ReLU backward
# ---------------------------------------------------------------------------------------------------------------------
def bn_bwd_ref(z, g1, g2, act, mean_t, invstd_t, gamma, G):
    """z, g1, g2 (or None), act (or None: g1 is already masked) as [G * n_pix, C] arrays of fp16 (act: fp16 or f32) VALUES;
    mean_t / invstd_t [G, C] and gamma [C] as the kernel gets them (float32).
    -> gy (float32: the fp16 tensor the kernel must store, bit for bit), gz (float64), dgamma, dbeta (float64, in the
    gradient tensors' loss-scaled units, the members added): O.clip_bwd and O.bn_train_bwd per member."""
    z = np.asarray(z, np.float32)
    n_pix, c = z.shape[0] // G, z.shape[1]
    gsum = np.asarray(g1, np.float32) + (np.asarray(g2, np.float32) if g2 is not None else 0)
    gy = r16(O.clip_bwd(np.asarray(act, np.float32), gsum) if act is not None else gsum)
    gz = np.empty(z.shape, np.float64)
    gg, gb = np.zeros(c), np.zeros(c)
    for m in range(G):
        sl = slice(m * n_pix, (m + 1) * n_pix)
        gx, g_g, g_b = O.bn_train_bwd(z[sl].astype(np.float64)[:, :, None, None], mean_t[m].astype(np.float64),
                                      invstd_t[m].astype(np.float64), gamma.astype(np.float64),
                                      gy[sl].astype(np.float64)[:, :, None, None])
        gz[sl] = gx[:, :, 0, 0]
        gg += g_g
        gb += g_b
    return gy, gz, gg, gb


def parity_scatter(g, h, w, fill=np.nan):
    """[B, h, w, C] -> the stride-2 data gradient's layout [B, ceil(h/2), ceil(w/2), 2, 2, C]: pixel (y, x) is parity class
    (y & 1, x & 1) of cell (y >> 1, x >> 1).  Cells past an odd edge are filled with `fill` (NaN: they must not be read)."""
    g = np.asarray(g)
    b, c = g.shape[0], g.shape[-1]
    out = np.full((b, (h + 1) // 2, (w + 1) // 2, 2, 2, c), fill, g.dtype)
    for a in range(2):
        for d in range(2):
            src = g[:, a::2, d::2]
            out[:, :src.shape[1], :src.shape[2], a, d] = src
    return out


def parity_gather(out, h, w):
    """the inverse: [B, ho, wo, 2, 2, C] -> [B, h, w, C]; the cells past an odd edge (garbage by contract) are dropped"""
    out = np.asarray(out)
    b, c = out.shape[0], out.shape[-1]
    g = np.empty((b, h, w, c), out.dtype)
    for a in range(2):
        for d in range(2):
            dst = g[:, a::2, d::2]
            dst[...] = out[:, :dst.shape[1], :dst.shape[2], a, d]
    return g


# ---------------------------------------------------------------------------------------------------------------------
# convolution backward
# ---------------------------------------------------------------------------------------------------------------------
def conv2d_bwd_ref(x, w, gy, stride, pad, ks=None, in_hw=None, dtype=torch.float64):
    """(gx, gw) of nn.Conv2d(bias=False) like O.conv2d_bwd (NCHW numpy in and out), through torch on the CPU, chunked over
    the batch.  gx needs w (x may be None: in_hw = (H, W) then); gw needs x (w may be None: ks then); what cannot be
    computed is returned as None.  dtype=torch.float32 is the plain float32 restatement the large-reduction bars come from."""
    _threads()
    gy = np.asarray(gy)
    b, co = gy.shape[:2]
    h, wd = (x.shape[2], x.shape[3]) if x is not None else in_hw
    gx = gw = wt = None
    if w is not None:
        wt = torch.from_numpy(np.ascontiguousarray(w)).to(dtype)
        ks = wt.shape[2]
        gx = np.empty((b, wt.shape[1], h, wd), np.float64 if dtype == torch.float64 else np.float32)
    # the im2col buffer of one image is the largest temporary: ci * ks * ks * ho * wo elements
    ci = wt.shape[1] if wt is not None else x.shape[1]
    per_img = 8 * (ci * ks * ks * gy.shape[2] * gy.shape[3] + 2 * gy[0].size + 2 * ci * h * wd)
    step = max(1, REF_CHUNK_BYTES // per_img)
    for i in range(0, b, step):
        g = torch.from_numpy(np.ascontiguousarray(gy[i:i + step])).to(dtype)
        if wt is not None:
            gx[i:i + step] = torch.nn.grad.conv2d_input((g.shape[0], ci, h, wd), wt, g, stride, pad).numpy()
        if x is not None:
            xs = torch.from_numpy(np.ascontiguousarray(x[i:i + step])).to(dtype)
            part = torch.nn.grad.conv2d_weight(xs, (co, ci, ks, ks), g, stride, pad)
            gw = part if gw is None else gw + part
    return gx, (gw.numpy() if gw is not None else None)


def wgrad_ref(x, gy, ks, stride, dtype=torch.float64):
    return conv2d_bwd_ref(x, None, gy, stride, ks // 2, ks=ks, dtype=dtype)[1]


def dgrad_ref(w, gy, stride, in_hw):
    return conv2d_bwd_ref(None, w, gy, stride, w.shape[2] // 2, in_hw=in_hw)[0]


def bar_from_restatement(floor, restated_err):
    """large reductions: 4 x the error of the plain float32 restatement against float64 (equally valid summation orders
    differ by small factors), never below the emulator suite's bar for the shape class"""
    return max(floor, 4.0 * restated_err)


# ---------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm statistics + normalise on the device: (C, n_pix per member, rows class, distribution); G = 3 everywhere.
#   one      rows == 1
#   mid      128 < rows < 768, rows % 128 != 0: the fold's `r += 128` loop with a ragged last step
#   cap      rows == 768, pixels per row not dividing n_pix (a short last row that still holds pixels)
#   cap+0    rows == 768 and trailing rows that cover no pixel (they must read as zeros)
#   bench    stage 1 of the bench batch: 256 * 80 * 32 pixels, C = 64 -- 5.2 M vectors per member: grid-stride normalise
STATS_CASES_GPU = [
    (64, 200, "one", "wide"),
    (128, 128 * 300 + 5, "mid", "wide"),
    (256, 60000, "cap", "wide"),
    (512, 768 * 32 + 1, "cap+0", "wide"),
    (64, 128 * 256 + 77, "mid", "offset"),          # mean 8, std 0.5: invstd from E[z^2] - mean^2 over f32 partial sums
    (64, 256 * 80 * 32, "bench", "wide"),
]


def check_rows_class(rows, n_pix, c, cls):
    assert rows == expected_rows(n_pix, c)[0], (rows, expected_rows(n_pix, c))
    empty = empty_trailing_rows(n_pix, c)
    if cls == "one":
        assert rows == 1
    elif cls == "mid":
        assert TF_FOLD_R < rows < TF_MAX_ROWS and rows % TF_FOLD_R != 0
    elif cls == "cap":
        assert rows == TF_MAX_ROWS and n_pix % expected_rows(n_pix, c)[1] != 0
    elif cls == "cap+0":
        assert rows == TF_MAX_ROWS and empty > 0
    elif cls == "bench":
        assert rows == TF_MAX_ROWS and n_pix * (c // 8) > TF_GRID_CAP * 256
    else:
        raise AssertionError(cls)


# Filter gradients on the device: (b, ci, co, h, w, ks, stride, loss scale, split class, S on a 256-CU device).  The split is
# S = min(ceil(CUs / ((co / 64) * (ci / 64))), n_tiles); the classes hold on a 256-CU device:
#   one    S == 1 (a single tile: nothing to fold)
#   tiles  1 < S < ceil(CUs / base): clipped to the tile count -- every split owns ONE tile, the last one short
#   cus    S == ceil(CUs / base) < 64
#   wide   S >= 64: the S-way fixed-order fold
WGRAD_CASES_GPU = [
    (32, 64, 64, 80, 32, 3, 1, 1024.0, "wide", 256),         # layer1: 256 splits over 81920 pixels
    (1, 64, 64, 80, 32, 3, 1, 256.0, "tiles", 10),
    (5, 64, 64, 25, 16, 3, 1, 256.0, "tiles", 9),          # odd map height
    (24, 128, 128, 40, 16, 3, 1, 1024.0, "wide", 64),       # layer2
    (1, 128, 128, 11, 8, 3, 1, 256.0, "one", 1),           # odd height, one tile
    (5, 256, 256, 20, 8, 3, 1, 1024.0, "tiles", 5),        # layer3
    (48, 256, 256, 20, 8, 3, 1, 256.0, "cus", 16),
    (1, 512, 512, 10, 4, 3, 1, 1024.0, "one", 1),          # layer4, one image: one tile
    (24, 512, 512, 10, 4, 3, 1, 256.0, "cus", 4),
    (128, 512, 512, 10, 4, 3, 1, 1024.0, "cus", 4),        # four splits of 1280 pixels each: the longest f32 accumulation
    (5, 64, 128, 80, 32, 5, 2, 1024.0, "tiles", 25),        # conv2
    (32, 64, 128, 80, 32, 5, 2, 256.0, "wide", 128),
    (3, 64, 128, 25, 16, 5, 2, 1024.0, "tiles", 3),        # odd input height
    (24, 128, 256, 40, 16, 5, 2, 256.0, "cus", 32),         # conv3
    (1, 128, 256, 11, 8, 5, 2, 1024.0, "one", 1),
    (5, 256, 512, 20, 8, 5, 2, 256.0, "tiles", 3),         # conv4
    (36, 256, 512, 20, 8, 5, 2, 1024.0, "cus", 8),
]


def check_split_class(S, cus, ci, co, cls, s256=None):
    """s256: the split of the case on a 256-CU device, as the host emulator plans it when told 256 CUs (for "tiles": the tile count)"""
    want = -(-cus // ((co // 64) * (ci // 64)))
    if cus == 256 and s256 is not None:
        assert S == s256, (S, s256)
    if cls == "one":
        assert S == 1
    elif cls == "tiles":
        assert 1 < S < want, (S, want)
    elif cls == "cus":
        assert S == want and S < 64, (S, want)
    elif cls == "wide":
        assert S >= 64, S
    else:
        raise AssertionError(cls)


# Data-gradient banks on the device: (b, ci, co, h, w) = the FORWARD layer's shape, [h, w] its input map
DGRAD3_CASES_GPU = [(4, 64, 64, 80, 32), (3, 64, 64, 25, 15), (4, 128, 128, 40, 16), (2, 128, 128, 11, 7),
                    (4, 256, 256, 20, 8), (5, 256, 256, 5, 3), (6, 512, 512, 10, 4), (3, 512, 512, 9, 3)]
DGRAD5_CASES_GPU = [(4, 64, 128, 80, 32), (3, 64, 128, 25, 15), (4, 128, 256, 40, 16), (2, 128, 256, 11, 7),
                    (6, 256, 512, 20, 8), (3, 256, 512, 19, 7)]
