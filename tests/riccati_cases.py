"""Inputs of the discrete-Riccati fixtures (tests/golden/riccati/, written by tools/make_riccati_fixtures.py).

Random systems are regenerated from their seed instead of being stored (an m = 300 system is megabytes of
incompressible draws); the fixture JSON keeps the SHA-256 of every regenerated array so that a NumPy whose
generator differs is caught instead of compared against outputs of other inputs.  The hand-built
systems are returned as they are.
"""
import hashlib

import numpy as np

# (m, n) of the random well-conditioned systems: A = 0.8 N / sqrt(m) (spectral radius about 0.8),
# Q = I + C C^T / (10 m), R = I + D D^T / n with C, D on a grid of 1/8 (so that C C^T is exact whatever
# the summation order of the BLAS that forms it)
RANDOM_SIZES = [(m, n) for m in (1, 2, 5, 14, 32, 64, 65, 128) for n in sorted({1, 3, m})] + [(300, 1), (300, 3)]


def random_case(m, n, seed):
    rng = np.random.default_rng(seed)
    A = 0.8 * rng.normal(size=(m, m)) / np.sqrt(m)
    B = rng.normal(size=(m, n))
    C = rng.integers(-4, 5, size=(m, m)) / 8.0
    Q = np.eye(m) + (C @ C.T) * (0.1 / m)
    D = rng.integers(-4, 5, size=(n, n)) / 8.0
    R = np.eye(n) + (D @ D.T) * (1.0 / n)
    return A, B, Q, R


def reference_problem():
    """tests/tensor/linalg/test_solvers/test_linear_control.py::test_solve_discrete_are_forward of the reference"""
    return (np.array([[4.0, 3.0], [-4.5, -3.5]]), np.array([[1.0], [-1.0]]), np.array([[9.0, 6.0], [6.0, 4.0]]),
            np.array([[1.0]]))


def seasonal_model():
    """Local level + 12-period dummy seasonal + two AR(1) states (m = 14, unit roots in the transition), observed
    through Z with noise H.  The steady-state prior covariance P of its Kalman filter solves the DARE in the
    filter's transposed form: P = solve_discrete_are(T^T, Z^T, R_q Q R_q^T, H).  Returns (T, Z, Qs, H)."""
    m = 14
    T = np.zeros((m, m))
    T[0, 0] = 1.0
    T[1, 1:12] = -1.0
    T[2:12, 1:11] = np.eye(10)
    T[12, 12] = 0.7
    T[13, 13] = 0.3
    Z = np.zeros((1, m))
    Z[0, [0, 1, 12, 13]] = 1.0
    Qs = np.diag([0.3, 0.05] + [0.0] * 10 + [0.2, 0.1])
    H = np.array([[1.0]])
    return T, Z, Qs, H


def unstabilizable():
    """the unstable mode 1.5 is not reached by B: no stabilising solution (the reference returns NaN)"""
    return np.diag([1.5, 0.5]), np.array([[0.0], [1.0]]), np.eye(2), np.eye(1)


def singular_r():
    """R = 0: the reference's compressed pencil still has a finite solution; the doubling algorithm needs R^-1"""
    rng = np.random.default_rng(1)
    return rng.normal(size=(4, 4)) * 0.4, rng.normal(size=(4, 1)), np.eye(4), np.zeros((1, 1))


def undetectable_scalar():
    """Q = 0 with an unstable A: (A, Q^1/2) is not detectable, yet the pair is stabilisable and the reference returns
    the stabilising (minimum-energy LQR) solution X = 3.  The doubling iteration stalls at H = 0 while Ak grows: NaN."""
    return np.array([[2.0]]), np.array([[1.0]]), np.array([[0.0]]), np.array([[1.0]])


def undetectable_2x2():
    """Q = diag(0, 1) leaves the unstable mode 1.2 unpenalised: the reference's solution is finite, the device's NaN"""
    return np.diag([1.2, 0.5]), np.array([[1.0], [1.0]]), np.diag([0.0, 1.0]), np.array([[1.0]])


def lyapunov_n0():
    """n = 0 (B has no columns): the DARE is the Stein equation X = A^T X A + Q"""
    return np.array([[0.5, 0.1], [0.0, 0.3]]), np.zeros((2, 0)), np.eye(2), np.zeros((0, 0))


SPECIAL = {"reference": reference_problem, "unstabilizable": unstabilizable, "singular_r": singular_r,
           "undetectable_scalar": undetectable_scalar, "undetectable_2x2": undetectable_2x2, "lyapunov_n0": lyapunov_n0}


def kalman_graph(pt, solve_discrete_are, scan):
    """steady-state Kalman filter log-likelihood of the seasonal model: P from the DARE, a Scan over the
    observations, parameters = the log standard deviations of the state noises and of the observation.
    Returns ([log_sd, y], logp)."""
    T, Z, _, _ = seasonal_model()
    log_sd = pt.dvector("log_sd")  # (level, seasonal, ar1, ar2, observation)
    y = pt.dvector("y")
    sd2 = pt.exp(2 * log_sd)
    idx = [0, 1, 12, 13]
    Qm = pt.zeros((14, 14), dtype="float64")
    Qm = Qm[idx, idx].set(sd2[:4])
    Hm = sd2[4].reshape((1, 1))
    Tt, Zt = pt.constant(T), pt.constant(Z)
    P = solve_discrete_are(Tt.T, Zt.T, Qm, Hm)  # steady-state prior covariance
    F = (Zt @ P @ Zt.T + Hm)[0, 0]
    K = (P @ Zt.T)[:, 0] / F  # steady-state gain

    def step(y_t, a, ll):
        v = y_t - (Zt @ a)[0]
        a_next = Tt @ (a + K * v)
        return a_next, ll - 0.5 * (np.log(2 * np.pi) + pt.log(F) + v ** 2 / F)

    a0, ll0 = pt.zeros(14, dtype="float64"), pt.constant(0.0, dtype="float64")
    (_, lls) = scan(step, sequences=[y], outputs_info=[a0, ll0], return_updates=False)
    return [log_sd, y], lls[-1]


def gradient_cost(pt, X, W):
    """the scalar whose gradient the gradient fixtures hold"""
    return (X * W).sum() + 0.5 * (X ** 2).sum()


def sha(arrays):
    return [hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() for a in arrays]


def case_inputs(meta):
    """(A, B, Q, R) of a fixture from its JSON entry; raises if a regenerated array differs from the recorded one"""
    kind = meta["kind"]
    if kind == "random":
        arrs = random_case(meta["m"], meta["n"], meta["seed"])
    elif kind == "seasonal":
        T, Z, Qs, H = seasonal_model()
        arrs = (T.T.copy(), Z.T.copy(), Qs, H)
    else:
        arrs = SPECIAL[kind]()
    got = sha(arrs)
    assert got == meta["sha256"], f"{meta['name']}: regenerated inputs differ from those the reference outputs were computed from"
    return arrs
