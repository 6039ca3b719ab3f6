"""The angular-margin softmax head (margin_head.hip) restated in NumPy, and the case tables of its two suites
(test_emul_margin_head.py on the host emulator, test_gpu_margin_head.py on the device, through margin_head_bodies.py).
A plain helper module: host arrays in, host arrays out; no GPU, no emulator, no fixtures.

`margin_ref` is the operation of include/deepspeaker_hip.h written from its definition -- forward and the closed-form
backward -- and takes `dtype`: np.float64 is the reference, np.float32 the plain restatement whose distance from the
reference sizes the bar (loss_side_cases.bar_from_restatement: max(floor, 4 x that distance), never the kernel's own
output).  test_emul_margin_head.py checks the float64 restatement itself against torch float64 autograd.

Floors: FLOOR_CE = 1e-6 for the loss and the log-sum-exp (the plain head's), FLOOR_COS = 1e-5 for c, the gradients and
the sums they are built from, in the rel_err sense (max |d| / max |ref|) of the plain head's tests.

Case tables: a trailing "gpu" marks a case only the device runs."""
import numpy as np

from deepspeaker_pytorch_amd._native import DS_MARGIN_SIN2_FLOOR as SIN2_FLOOR
from loss_side_cases import FLOOR_CE, bar_from_restatement, max_rel, rel_l2  # noqa: F401  (one definition for every suite)

F32, F64 = np.float32, np.float64
FLOOR_COS = 1e-5
KINDS = {"aam": 0, "am": 1}
DS_ERR_BAD_SHAPE, DS_ERR_ALIGNMENT, DS_ERR_NULL, DS_ERR_UNSUPPORTED = -1, -2, -3, -4
LABEL_COS_LIMIT = 0.99          # accuracy cases keep every label cosine inside it (the saturated plant is the exception)


def pad128(n):
    return -(-n // 128) * 128


def emul_cases(table):
    return [c for c in table if c[-1] != "gpu"]


def normalize_rows(a, dtype=F64):
    """(rows / norm, 1 / norm), both 0 for an all-zero row"""
    a = a.astype(dtype)
    nrm = np.sqrt((a * a).sum(1, dtype=dtype))
    inv = np.where(nrm > 0, dtype(1) / np.where(nrm > 0, nrm, dtype(1)), dtype(0)).astype(dtype)
    return a * inv[:, None], inv


def phi_of(c, m, kind, dtype=F64):
    """(phi, dphi/dc) of the label cosines c"""
    c, m = c.astype(dtype), dtype(m)
    one = np.ones_like(c)
    if kind == "am":
        return c - m, one
    sn = np.sqrt(np.maximum(dtype(1) - c * c, dtype(SIN2_FLOOR)))
    main = c > -np.cos(m)
    phi = np.where(main, c * np.cos(m) - sn * np.sin(m), c - m * np.sin(m))
    dphi = np.where(main, np.cos(m) + c * np.sin(m) / sn, one)
    return phi.astype(dtype), dphi.astype(dtype)


def margin_ref(x, w, labels, s, m, kind, gloss=1.0, dtype=F64):
    """forward and closed-form backward of the head; every array in `dtype`"""
    M, n = x.shape[0], w.shape[0]
    rows = np.arange(M)
    xh, inv_x = normalize_rows(x, dtype)
    wh, inv_w = normalize_rows(w, dtype)
    c = np.clip(xh @ wh.T, dtype(-1), dtype(1)).astype(dtype)
    phi, dphi = phi_of(c[rows, labels], m, kind, dtype)
    z = dtype(s) * c
    z[rows, labels] = dtype(s) * phi
    mx = z.max(1, keepdims=True)
    lse = (mx[:, 0] + np.log(np.exp(z - mx).sum(1, dtype=dtype))).astype(dtype)
    row_loss = lse - z[rows, labels]
    loss = dtype(row_loss.mean(dtype=F64))
    p = np.exp(z - lse[:, None])
    p[rows, labels] -= 1
    gc = (dtype(s) * (dtype(gloss) / dtype(M)) * p).astype(dtype)          # the clamp passes gradient everywhere
    gc[rows, labels] *= dphi
    r = (gc * c).sum(1, dtype=dtype)
    q = (gc * c).sum(0, dtype=dtype)
    gx = inv_x[:, None] * (gc @ wh - r[:, None] * xh)
    gw = inv_w[:, None] * (gc.T @ xh - q[:, None] * wh)
    return dict(xh=xh, wh=wh, inv_x=inv_x, inv_w=inv_w, c=c, lse=lse, row_loss=row_loss, loss=loss, gc=gc, r=r, q=q, gx=gx,
                gw=gw, label_cos=c[rows, labels])


def cosine_bwd_ref(x, w, gout, s, dtype=F64):
    """backward of out = s * clamp(cos(x, W)) for an incoming gradient gout [M, n_cls]"""
    xh, inv_x = normalize_rows(x, dtype)
    wh, inv_w = normalize_rows(w, dtype)
    c = np.clip(xh @ wh.T, dtype(-1), dtype(1))
    gc = dtype(s) * gout.astype(dtype)
    r, q = (gc * c).sum(1, dtype=dtype), (gc * c).sum(0, dtype=dtype)
    return inv_x[:, None] * (gc @ wh - r[:, None] * xh), inv_w[:, None] * (gc.T @ xh - q[:, None] * wh)


def label_plan(M, n_cls, rs):
    """labels at column 0, at n_cls - 1 (next to the padding) and, where there is one, in the second 128-column tile"""
    labels = rs.randint(0, n_cls, M).astype(np.int64)
    labels[0] = 0
    if M > 1:
        labels[M - 1] = n_cls - 1
    else:
        labels[0] = n_cls - 1
    if M > 2 and n_cls > 128:
        labels[1] = 128
    return labels


def _toward(w_row, cos, rs, gain):
    """a vector at cosine `cos` (sign included) to w_row, of norm |gain| * |w_row| / |cos|"""
    K = w_row.size
    u = w_row.astype(F64) / np.linalg.norm(w_row)
    v = rs.randn(K)
    v -= (v @ u) * u
    v /= np.linalg.norm(v)
    return (abs(gain) * np.linalg.norm(w_row) * (np.sign(cos) * u + np.sqrt(1 / cos ** 2 - 1) * v)).astype(F32)


def margin_inputs(M, n_cls, K, plant, seed):
    """x [M, K], W [n_cls, K] = 0.05 randn (label cosines |c| < 0.2 at K = 512, < 0.45 at K = 128), labels.  Plants:
    "fallback": row 0 at cosine -0.97 to its class row (x ~ -50 w_y: past theta = pi - m for every m > 0.25, ArcFace's
                fallback branch at m = 0.5), and row 1 at +0.89 (dphi/dc <= 1 + 7 sin m);
    "saturated": row 0 = 7 w_y exactly, c = 1 +- rounding;
    "zero": an all-zero x row (the last) and an all-zero class row (class 1, the label of row 1 where there is one);
    "padwin": every class row within 60 degrees of -u and every x near +u: all real cosines negative, so a pad column
              (c = 0) would be the row maximum if it were counted;
    "padwin_deep": the same with every cosine near -0.9, for scale 128: every s c lies below -104, so with a pad column
              as the row maximum every expf(z - 0) is 0 in float32 (e^-104 is under half the smallest denormal) and the
              log-sum-exp is -inf -- a pad column in the MAXIMUM shows, not only one in the sum."""
    rs = np.random.RandomState(seed)
    x = (rs.randn(M, K) * (0.3 + 3 * rs.rand(M, 1))).astype(F32)            # row norms differ by an order of magnitude
    w = (0.05 * rs.randn(n_cls, K)).astype(F32)
    labels = label_plan(M, n_cls, rs)
    if plant == "fallback":
        x[0] = _toward(w[labels[0]], -0.97, rs, 50.0)
        if M > 1:
            x[1] = _toward(w[labels[1]], 0.89, rs, 7.0)
    elif plant == "saturated":
        x[0] = F32(7) * w[labels[0]]
    elif plant == "zero":
        x[M - 1] = 0
        w[1 % n_cls] = 0
        if M > 2:
            labels[1] = 1 % n_cls
    elif plant in ("padwin", "padwin_deep"):
        u = rs.randn(K)
        u /= np.linalg.norm(u)
        spread = 1.0 if plant == "padwin" else 0.3
        w = (-u[None] + rs.randn(n_cls, K) * (spread * 0.8 / np.sqrt(K))).astype(F32)
        x = ((3 * u)[None] + rs.randn(M, K) * (spread * 1.5 / np.sqrt(K))).astype(F32)
    else:
        assert plant == "", plant
    return x, w, labels


# (M, n_cls, K, kind, margin, scale, plant, tag)
def _table():
    t = []
    kinds = ("aam", "am")
    # rows (four per workgroup, the 32-row GEMM tile plus one) x classes (the lane stride of 64, padding to 128 and 256)
    for i, M in enumerate((1, 3, 4, 5, 33)):
        for j, n in enumerate((2, 21, 64, 65, 127, 128, 129)):
            t.append((M, n, 512, kinds[(i + j) % 2], (0.2, 0.5)[(i + 2 * j) % 2], (30.0, 64.0, 1.0)[(i + j) % 3], "", ""))
    # the contraction: K % 128 == 0 (the data gradient's GEMM has K as its column count); 128 and 384 split 4 ways,
    # 256 and 512 split 8 ways -- the split counts fc_splits yields for such K
    for K in (128, 256, 384):
        t += [(5, 21, K, "aam", 0.2, 30.0, "", ""), (33, 129, K, "am", 0.5, 64.0, "", "")]
    # margin x scale x kind
    for m in (0.0, 0.2, 0.5):
        for s in (1.0, 30.0, 64.0):
            for kind in kinds:
                t.append((5, 129, 512, kind, m, s, "", ""))
    # edges
    for kind in kinds:
        t += [(5, 21, 512, kind, 0.5, 30.0, "fallback", ""), (5, 129, 512, kind, 0.2, 64.0, "fallback", ""),
              (4, 65, 512, kind, 0.2, 30.0, "saturated", ""), (5, 21, 512, kind, 0.2, 30.0, "zero", ""),
              (33, 21, 512, kind, 0.2, 64.0, "padwin", ""), (4, 127, 512, kind, 0.5, 64.0, "padwin", ""),
              (5, 21, 512, kind, 0.2, 128.0, "padwin_deep", ""), (4, 127, 512, kind, 0.2, 128.0, "padwin_deep", "")]
    # pre-training sizes: 3 x 256 rows, the classes of VoxCeleb1 and VoxCeleb2
    t += [(768, 1211, 512, "aam", 0.2, 30.0, "", "gpu"), (768, 5994, 512, "aam", 0.2, 30.0, "", "gpu")]
    return t


MARGIN_CASES = _table()
# The forward entry points take any K % 32 == 0 (only the data gradient's GEMM needs K % 128): K = 32, the smallest the
# GEMM accepts, and one K per split count fc_splits yields -- 32 and 96 -> 1 slice, 64 and 192 -> 2 -- forward only.
# (M, n_cls, K, kind, margin, scale, tag)
FORWARD_CASES = [(5, 21, 32, "aam", 0.2, 30.0, ""), (33, 129, 32, "am", 0.5, 64.0, ""), (5, 129, 64, "aam", 0.5, 30.0, ""),
                 (33, 21, 64, "am", 0.2, 1.0, ""), (4, 65, 96, "aam", 0.2, 64.0, ""), (3, 128, 192, "am", 0.2, 30.0, "")]
EXPECTED_S = {32: 1, 64: 2, 96: 1, 192: 2, 128: 4, 256: 8, 384: 4, 512: 8}
