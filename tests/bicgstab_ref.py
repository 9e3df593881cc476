"""CPU restatement of the BiCGStab the library runs: PETSc KSPBCGS, left preconditioning, zero
initial guess (the recurrence in the header of csrc/bicgstab.hip, formula for formula).

    bcgs(mult, pc, b, rtol, atol, max_it, dot=np.dot, hist=None) -> (x, info)

mult and pc are callables (pc None: the identity); hist, a list, collects (x_k, dp_k) per iteration.
rdot is a second dot with another rounding pattern (the products summed in reversed blocks of
1,024): together with ``Ac.to_scipy() @ x`` in place of ``Ac.mult`` it gives a second restatement, and
the distance between the two says how far rounding alone scatters the iterates of a case.
"""
import numpy as np


def rdot(a, b):
    """(a, b) with the products summed block by block (1,024 entries, each block reversed), last block first."""
    pr = a * b
    tot = 0.0
    for lo in reversed(range(0, len(pr), 1024)):
        tot += float(np.sum(pr[lo:lo + 1024][::-1]))
    return tot


def bcgs(mult, pc, b, rtol, atol, max_it, dot=np.dot, hist=None):
    if pc is None:
        pc = lambda y: y  # noqa: E731
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros_like(b)
    r = np.array(pc(b), dtype=np.float64)
    rh = r.copy()
    dp = float(np.sqrt(dot(r, r)))
    info = dict(converged=False, iterations=0, initial_norm=dp, final_norm=dp, breakdown=None)
    ttol = max(rtol * dp, atol)
    if dp <= ttol or dp == 0.0:
        info["converged"] = True
        return x, info
    if max_it <= 0:
        return x, info
    rho_old = alpha = omega_old = 1.0
    p = np.zeros_like(b)
    v = np.zeros_like(b)
    for i in range(max_it):
        rho = float(dot(r, rh))
        if rho == 0.0:
            info["breakdown"] = "rho"
            break
        beta = (rho / rho_old) * (alpha / omega_old)
        p = r + beta * (p - omega_old * v)
        v = np.asarray(pc(mult(p)))
        d1 = float(dot(v, rh))
        if d1 == 0.0:
            info["breakdown"] = "d1"
            break
        alpha = rho / d1
        s = r - alpha * v
        t = np.asarray(pc(mult(s)))
        d1 = float(dot(s, t))
        d2 = float(dot(t, t))
        if d2 == 0.0:
            x = x + alpha * p
            info["iterations"] = i + 1
            info["final_norm"] = dp = 0.0
            if float(dot(s, s)) == 0.0:
                info["converged"] = True
            else:
                info["breakdown"] = "d2"
            if hist is not None:
                hist.append((x.copy(), dp))
            break
        omega = d1 / d2
        x = x + alpha * p + omega * s
        r = s - omega * t
        dp = float(np.sqrt(dot(r, r)))
        rho_old, omega_old = rho, omega
        info["iterations"] = i + 1
        info["final_norm"] = dp
        if hist is not None:
            hist.append((x.copy(), dp))
        if dp <= ttol:
            info["converged"] = True
            break
        if i + 1 >= max_it or not np.isfinite(dp):
            break
    return x, info


def restatements(Ac, Bo, pc, pc2=None, rtol=0.0, atol=0.0, max_it=8):
    """The two restatements of one system: (x, info, hist) with Ac.mult and np.dot, and with the scipy
    product and rdot."""
    S = Ac.to_scipy()
    h1, h2 = [], []
    x1, i1 = bcgs(Ac.mult, pc, Bo, rtol, atol, max_it, hist=h1)
    x2, i2 = bcgs(lambda y: S @ y, pc2 if pc2 is not None else pc, Bo, rtol, atol, max_it, dot=rdot, hist=h2)
    return (x1, i1, h1), (x2, i2, h2)


def drift(h1, h2):
    """Largest relative distance between two histories' iterates (over the common length)."""
    return max((np.linalg.norm(a - b) / np.linalg.norm(a) for (a, _), (b, _) in zip(h1, h2)), default=0.0)
