"""The rules of representation similarity (copo_amd/eval/similarity.py, copo_hidden_obs_seats_f32, copo_cka_accumulate, copo_cka_finish;
DESIGN.md section 8w) restated in float64 numpy: the hidden layers, the mask of counted positions, the accumulators S / s / n, the
centred HSIC, linear CKA and the unit statistics.  No GPU and no native library."""
import numpy as np

F_ACTED = 0x01                  # COPO_F_ACTED
DEAD_VARIANCE, SATURATED_MEAN = 1e-8, 0.99


def hidden64(net, obs):
    """(h1, h2) float64 [n][H] of a net (W1, b1, W2, b2, W3, b3), weights [out][in], on the rows of obs."""
    W1, b1, W2, b2 = (np.asarray(a, np.float64) for a in net[:4])
    h1 = np.tanh(np.asarray(obs, np.float64) @ W1.T + b1)
    return h1, np.tanh(h1 @ W2.T + b2)


def heads64(net, h2):
    """[n][4] float64: W3 h2 + b3."""
    return np.asarray(h2, np.float64) @ np.asarray(net[4], np.float64).T + np.asarray(net[5], np.float64)


def common_rows(seat, group, G):
    """The ascending list of the seated rows e N + n of the scene groups in [0, G)."""
    seat, group = np.asarray(seat), np.asarray(group)
    ok = (seat >= 0) & ((group >= 0) & (group < G))[:, None]
    return np.nonzero(ok.reshape(-1))[0].astype(np.int64)


def counted(rows, count, flags, seat, rows_of):
    """bool [len(rows)]: position p counts when p < count, 0 <= rows[p] < n_out, flags[rows[p]] carry ACTED and (rows_of < 0 or
    seat[rows[p]] == rows_of)."""
    rows, flags, seat = np.asarray(rows, np.int64), np.asarray(flags).reshape(-1), np.asarray(seat).reshape(-1)
    ok = (np.arange(len(rows)) < int(count)) & (rows >= 0) & (rows < len(flags))
    r = np.where(ok, rows, 0)
    ok &= (flags[r] & F_ACTED) != 0
    if rows_of is not None and int(rows_of) >= 0:
        ok &= seat[r] == int(rows_of)
    return ok


def accumulate(hidden, panel, mask, acc=None):
    """One step added to acc = dict(S [P][2][H][H], s [M][2][H], n): `hidden` [K][cap][2][H] (any float dtype, read as float64; whatever
    it holds at positions outside `mask` is never touched), `panel` the members compared, pairs a <= b in row-major order."""
    hidden, mask = np.asarray(hidden), np.asarray(mask, bool)
    M, H = len(panel), hidden.shape[3]
    if acc is None:
        acc = dict(S=np.zeros((M * (M + 1) // 2, 2, H, H), np.float64), s=np.zeros((M, 2, H), np.float64), n=0)
    h = [hidden[int(m)][mask].astype(np.float64) for m in panel]          # [M] x [n][2][H]
    pair = 0
    for a in range(M):
        for b in range(a, M):
            for layer in range(2):
                acc["S"][pair, layer] += h[a][:, layer].T @ h[b][:, layer]
            pair += 1
        acc["s"][a] += h[a].sum(axis=0)
    acc["n"] += int(mask.sum())
    return acc


def pair_index(a, b, M):
    a, b = min(a, b), max(a, b)
    return a * M - a * (a - 1) // 2 + (b - a)


def hsic(acc, M):
    """[M][M][2] float64: || S[a,b,l] - s[a,l] s[b,l]^T / n ||_F^2, both triangles; zeros with n < 2."""
    out = np.zeros((M, M, 2), np.float64)
    if acc["n"] < 2:
        return out
    for a in range(M):
        for b in range(a, M):
            for layer in range(2):
                d = acc["S"][pair_index(a, b, M), layer] - np.outer(acc["s"][a, layer], acc["s"][b, layer]) / acc["n"]
                out[a, b, layer] = out[b, a, layer] = float((d * d).sum())
    return out


def cka(hs, n):
    """[M][M][2]: hsic[a][b] / sqrt(hsic[a][a] hsic[b][b]); NaN with n < 2 or a zero norm."""
    hs = np.asarray(hs, np.float64)
    M = hs.shape[0]
    out = np.full(hs.shape, np.nan)
    if n < 2:
        return out
    for a in range(M):
        for b in range(M):
            for layer in range(2):
                den = hs[a, a, layer] * hs[b, b, layer]
                if den > 0.0:
                    out[a, b, layer] = hs[a, b, layer] / np.sqrt(den)
    return out


def cka_of_activations(X, Y):
    """Linear CKA of two activation matrices [n][p], [n][q] straight from the definition (centred features), float64."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    if X.shape[0] < 2:
        return float("nan")
    X, Y = X - X.mean(axis=0), Y - Y.mean(axis=0)
    den = np.sqrt(((X.T @ X) ** 2).sum() * ((Y.T @ Y) ** 2).sum())
    return float(((X.T @ Y) ** 2).sum() / den) if den > 0.0 else float("nan")


def unit_stats(acc, M):
    """(mean [M][2][H], var [M][2][H]): s / n and diag(S[a,a,l]) / n - mean^2; zeros with n < 2."""
    H = acc["s"].shape[2]
    mean, var = np.zeros((M, 2, H)), np.zeros((M, 2, H))
    if acc["n"] < 2:
        return mean, var
    for a in range(M):
        for layer in range(2):
            mean[a, layer] = acc["s"][a, layer] / acc["n"]
            var[a, layer] = np.diag(acc["S"][pair_index(a, a, M), layer]) / acc["n"] - mean[a, layer] ** 2
    return mean, var


def census(mean, var):
    """(dead_units, saturated_units, mean_abs_activation) of one (member, layer)."""
    return int((var < DEAD_VARIANCE).sum()), int((np.abs(mean) > SATURATED_MEAN).sum()), float(np.abs(mean).mean())
