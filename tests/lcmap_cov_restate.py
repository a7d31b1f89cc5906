"""A numpy restatement of the landmark map's two options (xivo_hip_lcmap_cov_config), written from the header's text, not from
the kernels: the visit rule - which matches rest, whether the frame closes, what every matched entry remembers - and the
point covariance in the gate and in the rows (R_e = Rlc I + H_T Sigma H_T^T, gamma on the unwhitened pair, L^-1 times the pair).
The rows themselves are tests/lcmap_restate.py's. The host driver (tests/lcmap_cov_driver.cpp, the integer rules of
lcmap_device.h) and the GPU tests are held against it."""
import numpy as np

import lcmap_restate as R

NONE, SHORT, CLOSED, RESTED = range(4)
COV_STATS = ("resting", "rested_frames", "bad_cov")
SYM6 = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def pack6(S):
    return np.array([S[r, c] for r, c in SYM6])


def unpack6(v):
    S = np.zeros((3, 3))
    for k, (r, c) in enumerate(SYM6):
        S[r, c] = S[c, r] = v[k]
    return S


class VisitRestate:
    """one filter's map with the visit rule: keys in entry order, per entry last_seen (0: never) and used; t counts the calls"""

    def __init__(self, map_max, lc_max, min_matches, gap):
        self.map_max, self.lc_max, self.min_matches, self.gap = map_max, lc_max, min_matches, gap
        self.keys, self.last_seen, self.used = [], [], []
        self.t = 0
        self.stats = dict.fromkeys(COV_STATS + ("gated", "short_frames", "closed_frames"), 0)

    def add(self, keys):
        for k in keys:
            if k >= 0 and k not in self.keys and len(self.keys) < self.map_max:
                self.keys.append(k); self.last_seen.append(0); self.used.append(0)

    def close(self, qkeys, kept):
        """qkeys: the call's query keys in order; kept: the gate's answer per list position (a list, or a function of the
        position). -> dict(entries, resting, kept, frame, neutral [lc_max], n_fresh)"""
        self.t += 1
        lst = [self.keys.index(k) for k in qkeys if k >= 0 and k in self.keys][:self.lc_max]
        n = len(lst)
        kp = [bool(kept(m) if callable(kept) else kept[m]) for m in range(n)]
        # every position sees the state from before the call
        used_now = [self.used[e] if (self.last_seen[e] > 0 and self.t - self.last_seen[e] <= self.gap) else 0 for e in lst]
        resting = [self.gap > 0 and bool(u) for u in used_now]
        n_kept = sum(kp); n_fresh = sum(k and not r for k, r in zip(kp, resting))
        if n_kept >= self.min_matches and n_kept > 0:
            frame = CLOSED if n_fresh > 0 else RESTED
        else:
            frame = SHORT if n > 0 else NONE
        neutral = [not (frame == CLOSED and m < n and kp[m] and not resting[m]) for m in range(self.lc_max)]
        nxt = {}
        for m, e in enumerate(lst):                          # a key at two positions: used if either used it
            nxt[e] = nxt.get(e, 0) or int(bool(used_now[m]) or (frame == CLOSED and kp[m] and not resting[m]))
        for e, u in nxt.items():
            self.last_seen[e], self.used[e] = self.t, u
        st = self.stats
        st["gated"] += n - n_kept; st["short_frames"] += frame == SHORT; st["closed_frames"] += frame == CLOSED
        st["rested_frames"] += frame == RESTED; st["resting"] += sum(k and r for k, r in zip(kp, resting))
        return dict(entries=lst, resting=[int(r) for r in resting], kept=[int(k) for k in kp], frame=frame,
                    neutral=[int(v) for v in neutral], n_fresh=n_fresh)


def r_eff(Hi, Sigma, Rlc, goff=0):
    """R_e = Rlc I + H_T Sigma H_T^T of one pair, H_T its block for Tsb: columns goff + 3 .. goff + 5 (d xp / d Xs = -H_T)"""
    HT = Hi[:, goff + 3:goff + 6]
    return Rlc * np.eye(2) + HT @ Sigma @ HT.T


def pivots_ok(S):
    return bool(S[0, 0] > 0 and S[1, 1] - S[1, 0] ** 2 / S[0, 0] > 0)


def gamma(Hi, P, r, Re):
    """r^T (H_i P H_i^T + R_e)^-1 r on the unwhitened pair; None where R_e or the sum has a non-positive pivot, or the value is
    not finite (lcmap_restate.kept: never kept)"""
    S = Hi @ P @ Hi.T + Re
    if not pivots_ok(Re) or not pivots_ok(S):
        return None
    with np.errstate(all="ignore"):
        g = float(r @ np.linalg.solve(S, r))
    return g if np.isfinite(g) else None


def whiten(H, inn, dR, Res, neutral):
    """the staged rows: L^-1 times every pair that takes part (R_e = L L^T), diagR = 1; the neutral pairs zero"""
    H, inn, dR = R.neutralise(H, inn, dR, neutral)
    for m, nt in enumerate(neutral):
        if not nt:
            L = np.linalg.cholesky(Res[m])
            H[2 * m:2 * m + 2] = np.linalg.solve(L, H[2 * m:2 * m + 2]); inn[2 * m:2 * m + 2] = np.linalg.solve(L, inn[2 * m:2 * m + 2])
            dR[2 * m:2 * m + 2] = 1.0
    return H, inn, dR


def joseph_full_R(H, P, inn, Re):
    """the Joseph form with a full R: K = P H^T (H P H^T + R)^-1, dx = K inn, P+ = (I - K H) P (I - K H)^T + K R K^T"""
    K = P @ H.T @ np.linalg.inv(H @ P @ H.T + Re)
    A = np.eye(P.shape[0]) - K @ H
    return K @ inn, A @ P @ A.T + K @ Re @ K.T


def block_R(Res, neutral, lc_max):
    """block-diagonal R of all lc_max pairs: R_e of the pairs that take part, the identity on the neutral ones"""
    Re = np.eye(2 * lc_max)
    for m in range(lc_max):
        if not neutral[m]:
            Re[2 * m:2 * m + 2, 2 * m:2 * m + 2] = Res[m]
    return Re
