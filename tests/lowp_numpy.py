"""The rules of the low-precision policy forward (copo_lowp_pack, copo_lowp_forward_seats, copo_amd/eval/precision.py; DESIGN.md section
8t) restated in numpy.  No GPU and no native library is touched at import.

A format p is "bfloat16" or "float8_e4m3" (OCP e4m3fn: no infinities, largest value 448).
  rnd_p        round to nearest even into p; e4m3 clamps to [-448, 448] first; subnormals are kept
  weights      per layer l in {1, 2, 3} and output unit u: s_l[u] = 1 (bfloat16) or 2^ceil(log2(max_k |W_l[u][k]| / 448)), 1 for a zero row
               (e4m3); q_l[u][k] = rnd_p(W_l[u][k] / s_l[u]); biases: fp32 (e4m3), rnd_bf16 (bfloat16)
  a row o      x = rnd_p(o); h1 = rnd_p(tanh(rz(s_1 (q_1 x) + b_1))); h2 alike from h1; out = rz(s_3 (q_3 h2) + b_3); rz = rnd_bf16 for
               bfloat16 -- the places where the bfloat16 operand mode of the learner's forward rounds -- and the identity for e4m3
"""
import numpy as np

FORMATS = ("bfloat16", "float8_e4m3")
E4M3_MAX = 448.0
F = np.float32


def rnd_bf16(x):
    """float32 -> the nearest bfloat16 (ties to even), as float32."""
    u = np.ascontiguousarray(x, F).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(F).reshape(np.shape(x))


def rnd_e4m3(x):
    """float -> the nearest e4m3 value of clamp(x, -448, 448) (ties to even; steps of 2^-9 below 2^-6), as float32.  Exact in float64."""
    a = np.minimum(np.abs(np.asarray(x, np.float64)), E4M3_MAX)
    with np.errstate(divide="ignore"):
        e = np.maximum(np.floor(np.log2(np.where(a > 0, a, 1.0))), -6.0)
    step = np.exp2(e - 3.0)
    return np.copysign(np.rint(a / step) * step, x).astype(F)         # (np.rint rounds halves to even; -0 keeps its sign)


def rnd(fmt, x):
    return rnd_bf16(np.asarray(x, F)) if fmt == "bfloat16" else rnd_e4m3(x)


def row_scales(fmt, W):
    """s [units] float32 of a weight matrix [units][k]."""
    amax = np.abs(np.asarray(W, np.float64)).max(axis=1)
    if fmt == "bfloat16":
        return np.ones(len(amax), F)
    s = np.ones(len(amax), np.float64)
    for u, m in enumerate(amax):
        if m > 0 and np.isfinite(m):
            e = int(np.ceil(np.log2(m / E4M3_MAX)))
            while m / 2.0 ** e > E4M3_MAX:          # (the logarithm is only a first guess: these two loops make it exact)
                e += 1
            while m / 2.0 ** (e - 1) <= E4M3_MAX:
                e -= 1
            s[u] = 2.0 ** min(max(e, -126), 127)
    return s.astype(F)


def quantise(fmt, net):
    """(W1, b1, W2, b2, W3, b3) float32 -> dict q1 q2 q3 s1 s2 s3 b1 b2 b3 (float32 values)."""
    out = {}
    for l in (1, 2, 3):
        W, b = np.asarray(net[2 * l - 2], F), np.asarray(net[2 * l - 1], F)
        s = row_scales(fmt, W)
        out["s%d" % l], out["q%d" % l] = s, rnd(fmt, (W / s[:, None]).astype(F))
        out["b%d" % l] = rnd_bf16(b) if fmt == "bfloat16" else b
    return out


# ---- the packed image ------------------------------------------------------------------------------------------------------------
def k1p_of(in_dim):
    return (int(in_dim) + 31) // 32 * 32


def image_bytes(fmt, hidden, in_dim):
    return hidden * (k1p_of(in_dim) + hidden) * (2 if fmt == "bfloat16" else 1) + 4 * (8 * hidden + 8)


def encode(fmt, v):
    """Values of the format (float32) -> their codes: uint16 (bfloat16) or uint8 (e4m3)."""
    v = np.ascontiguousarray(v, F)
    if fmt == "bfloat16":
        return (v.view(np.uint32) >> 16).astype(np.uint16)
    a = np.abs(v.astype(np.float64))
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    normal = a >= 2.0 ** -6
    code = np.where(normal, ((e + 7).astype(np.int64) << 3) | np.rint((a / np.exp2(e) - 1.0) * 8).astype(np.int64), np.rint(a * 512).astype(np.int64))
    return (code | (np.signbit(v).astype(np.int64) << 7)).astype(np.uint8)


def decode(fmt, c):
    if fmt == "bfloat16":
        return (np.asarray(c, np.uint32) << 16).view(F)
    c = np.asarray(c, np.int64)
    e, m = (c >> 3) & 15, c & 7
    a = np.where(e == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * np.exp2(e - 7.0))
    return (np.where(c & 0x80, -a, a)).astype(F)


def pack_image(fmt, net):
    """The bytes copo_lowp_pack writes for one member: q1 [H][K1P], q2 [H][H] (codes, k contiguous, zero beyond in_dim), then float32
    q3 [4][H], s1, s2, s3 [4], b1, b2, b3 [4]."""
    q = quantise(fmt, net)
    H, K1 = q["q1"].shape
    q1 = np.zeros((H, k1p_of(K1)), F)
    q1[:, :K1] = q["q1"]
    tail = np.concatenate([q[k].reshape(-1) for k in ("q3", "s1", "s2", "s3", "b1", "b2", "b3")]).astype(F)
    return np.concatenate([encode(fmt, q1).reshape(-1).view(np.uint8), encode(fmt, q["q2"]).reshape(-1).view(np.uint8), tail.view(np.uint8)])


def unpack_image(fmt, img, hidden, in_dim):
    """The inverse of `pack_image`, the padding included: dict q1 [H][K1P] ... as float32 values."""
    H, KP, esz = hidden, k1p_of(in_dim), 2 if fmt == "bfloat16" else 1
    dt = np.uint16 if esz == 2 else np.uint8
    n1, n2 = H * KP * esz, H * H * esz
    f = img[n1 + n2:n1 + n2 + 4 * (8 * H + 8)].view(F)
    cut = np.cumsum([0, 4 * H, H, H, 4, H, H, 4])
    parts = {k: f[cut[i]:cut[i + 1]] for i, k in enumerate(("q3", "s1", "s2", "s3", "b1", "b2", "b3"))}
    parts["q3"] = parts["q3"].reshape(4, H)
    parts["q1"] = decode(fmt, img[:n1].view(dt)).reshape(H, KP)
    parts["q2"] = decode(fmt, img[n1:n1 + n2].view(dt)).reshape(H, H)
    return parts


# ---- the forward -----------------------------------------------------------------------------------------------------------------
def forward64(fmt, net, obs):
    """[n][4] float64: the spec with every sum in float64."""
    q = quantise(fmt, net)
    rz = (lambda z: rnd_bf16(z.astype(F)).astype(np.float64)) if fmt == "bfloat16" else (lambda z: z)
    d = lambda a: np.asarray(a, np.float64)  # noqa: E731
    h = d(rnd(fmt, np.asarray(obs, F)))
    for l in (1, 2):
        z = rz(d(q["s%d" % l]) * (h @ d(q["q%d" % l]).T) + d(q["b%d" % l]))
        h = d(rnd(fmt, np.tanh(z).astype(F)))
    return rz(d(q["s3"]) * (h @ d(q["q3"]).T) + d(q["b3"]))


def forward32_chunked(fmt, net, obs, chunk=32):
    """[n][4] float32: the same spec with every sum in float32, `chunk` terms at a time in order, the chunks added in order."""
    q = quantise(fmt, net)
    rz = rnd_bf16 if fmt == "bfloat16" else (lambda z: z)

    def dot(h, W):
        acc = np.zeros((h.shape[0], W.shape[0]), F)
        for k0 in range(0, h.shape[1], chunk):
            part = np.zeros_like(acc)
            for k in range(k0, min(k0 + chunk, h.shape[1])):
                part = (part + (h[:, k:k + 1] * W[None, :, k]).astype(F)).astype(F)
            acc = (acc + part).astype(F)
        return acc

    h = rnd(fmt, np.asarray(obs, F))
    for l in (1, 2):
        z = rz(((q["s%d" % l] * dot(h, q["q%d" % l])).astype(F) + q["b%d" % l]).astype(F))
        h = rnd(fmt, np.tanh(z.astype(np.float64)).astype(F))
    return rz(((q["s3"] * dot(h, q["q3"])).astype(F) + q["b3"]).astype(F))


def sign_net64(net, obs):
    """[n][4] float64: W3 sgn(W2 sgn(W1 o + b1) + b2) + b3, what the exact case's networks compute when tanh saturates."""
    W1, b1, W2, b2, W3, b3 = (np.asarray(a, np.float64) for a in net)
    return np.sign(np.sign(np.asarray(obs, np.float64) @ W1.T + b1) @ W2.T + b2) @ W3.T + b3
