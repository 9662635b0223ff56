"""Closed forms a simulated queueing net is put beside (plain numpy, textbook formulas: e.g. Gross & Harris,
*Fundamentals of Queueing Theory*, sections 2.5 M/M/1/K, 2.6 M/M/c/K, 4.2 open Jackson networks).  The counterpart of
the validation harness the reference's simulator ends in (``calculate_theoretical_renege_rate``); the simulation side is
``simulation_v3.mm1k_sweep``.

Notation: arrival rate ``lam``, service rate ``mu`` per server, ``queue_cap`` waiting places (what the simulator's
``queue_list`` holds), so a single-server station holds at most K = queue_cap + 1 customers."""
import math

import numpy as np


def mm1k(lam, mu, queue_cap):
    """M/M/1/K with K = queue_cap + 1 -> dict:
      p           (K + 1) stationary probabilities of n = 0..K customers in the station: p[n] ~ rho**n, rho = lam / mu
                  (uniform for rho == 1: the weights are all 1, no 0 / 0 is formed)
      blocking    p[K]: the fraction of arrivals that find the station full (PASTA)
      utilisation 1 - p[0]
      L, LQ       mean number in the station / waiting: sum n p[n], sum (n - 1) p[n] over n >= 1
      W, WQ       Little's law with the ACCEPTED rate lam (1 - p[K]): the mean time of a customer who was admitted
      queue_length_probabilities  (queue_cap + 1): the law of the number WAITING, (p[0] + p[1], p[2], ..., p[K])"""
    lam, mu, queue_cap = float(lam), float(mu), int(queue_cap)
    if not (lam > 0 and mu > 0 and queue_cap >= 0):
        raise ValueError("mm1k: lam > 0, mu > 0 and queue_cap >= 0 are required")
    k = queue_cap + 1
    n = np.arange(k + 1, dtype=np.float64)
    w = (lam / mu) ** n
    p = w / w.sum()
    accepted = lam * (1.0 - p[k])
    big_l = float((n * p).sum())
    lq = float(((n[1:] - 1.0) * p[1:]).sum())
    return {"p": p, "blocking": float(p[k]), "utilisation": float(1.0 - p[0]), "L": big_l, "LQ": lq,
            "W": big_l / accepted, "WQ": lq / accepted,
            "queue_length_probabilities": np.concatenate([[p[0] + p[1]], p[2:]])}


def _mm1k_erlang_mixture(lam, mu, queue_cap, t, more):
    """sum over n = 0 .. K - 1 of q[n] * P(Erlang(n + more, mu) > t), q[n] = p[n] / (1 - p[K]): what an ACCEPTED arrival
    finds (PASTA, conditioned on not being turned away) and the n + more exponential stages it then sits through;
    P(Erlang(m, mu) > t) = sum over j < m of exp(-mu t) (mu t)**j / j!  (0 for m = 0)."""
    p = mm1k(lam, mu, queue_cap)["p"]
    k = len(p) - 1
    q = p[:k] / (1.0 - p[k])
    x = float(mu) * np.asarray(t, dtype=np.float64)
    if (x < 0).any():
        raise ValueError("mm1k waiting-time tails: t >= 0 is required")
    term = [np.exp(-x) * x ** j / math.factorial(j) for j in range(k - 1 + more)]
    out = np.zeros_like(x)
    for n in range(k):
        for j in range(n + more):
            out = out + q[n] * term[j]
    return out


def mm1k_wait_tail(lam, mu, queue_cap, t):
    """P(Wq > t) of a customer ADMITTED to M/M/1/K (FIFO), K = queue_cap + 1, for t >= 0 (a scalar or an array -> the
    same shape): sum over n = 1 .. K - 1 of q[n] * sum over j < n of exp(-mu t) (mu t)**j / j!, q[n] = p[n] / (1 - p[K])
    with ``mm1k``'s p -- an arrival that finds n customers waits for n exponential completions (the one in service is
    memoryless), a mixture of Erlang laws (e.g. Gross & Harris, section 2.5, the waiting-time distribution of the
    finite queue).  At t = 0 it is 1 - q[0], the chance of waiting at all.  The simulated counterpart is
    ``simulation_v3.mm1k_wait_sweep``."""
    return _mm1k_erlang_mixture(lam, mu, queue_cap, t, 0)


def mm1k_sojourn_tail(lam, mu, queue_cap, t):
    """P(W > t) of an admitted customer's whole time in the station: ``mm1k_wait_tail`` with one more stage, the
    customer's own service -- sum over n = 0 .. K - 1 of q[n] * sum over j <= n of exp(-mu t) (mu t)**j / j!."""
    return _mm1k_erlang_mixture(lam, mu, queue_cap, t, 1)


def mmck_blocking(lam, mu, c, queue_cap):
    """The blocking probability of M/M/c/N, N = c + queue_cap: p[N] with p[n] ~ a**n / n! for n <= c and
    a**n / (c! c**(n - c)) beyond, a = lam / mu.  c = 1 is ``mm1k(...)["blocking"]``.  The simulated counterpart is a
    ``['queue']`` node in front of c servers (``simulation_v3.mmck_spec`` / ``mmck_sweep``), which holds one customer
    even with capacity 0: compare it with ``queue_cap = max(queue_list, 1)``; ``mmck`` below is the full law."""
    lam, mu, c, queue_cap = float(lam), float(mu), int(c), int(queue_cap)
    if not (lam > 0 and mu > 0 and c >= 1 and queue_cap >= 0):
        raise ValueError("mmck_blocking: lam > 0, mu > 0, c >= 1 and queue_cap >= 0 are required")
    a, big_n = lam / mu, c + queue_cap
    w = [a ** n / math.factorial(n) if n <= c else a ** n / (math.factorial(c) * float(c) ** (n - c))
         for n in range(big_n + 1)]
    return w[big_n] / math.fsum(w)


def mmck(lam, mu, c, queue_cap):
    """M/M/c/N with N = c + queue_cap -> the dict of ``mm1k``:
      p           (N + 1) stationary probabilities, p[n] ~ a**n / n! for n <= c and a**n / (c! c**(n - c)) beyond
      blocking    p[N]
      utilisation PER SERVER: the mean number of busy servers, sum min(n, c) p[n], over c
      L, LQ       mean number in the station / waiting: sum n p[n], sum (n - c) p[n] over n > c
      W, WQ       Little's law with the accepted rate lam (1 - p[N])
      queue_length_probabilities  (queue_cap + 1): the law of the number waiting, (p[0] + .. + p[c], p[c + 1], .., p[N])
    c = 1 is ``mm1k`` (the same weights; the utilisation is summed here and 1 - p[0] there)."""
    lam, mu, c, queue_cap = float(lam), float(mu), int(c), int(queue_cap)
    if not (lam > 0 and mu > 0 and c >= 1 and queue_cap >= 0):
        raise ValueError("mmck: lam > 0, mu > 0, c >= 1 and queue_cap >= 0 are required")
    a, big_n = lam / mu, c + queue_cap
    n = np.arange(big_n + 1, dtype=np.float64)
    w = np.array([a ** i / math.factorial(i) if i <= c else a ** i / (math.factorial(c) * float(c) ** (i - c))
                  for i in range(big_n + 1)], dtype=np.float64)
    p = w / w.sum()
    accepted = lam * (1.0 - p[big_n])
    big_l = float((n * p).sum())
    lq = float(((n[c:] - c) * p[c:]).sum())
    return {"p": p, "blocking": float(p[big_n]), "utilisation": float((np.minimum(n, c) * p).sum() / c), "L": big_l,
            "LQ": lq, "W": big_l / accepted, "WQ": lq / accepted,
            "queue_length_probabilities": np.concatenate([[p[:c + 1].sum()], p[c + 1:]])}


def mean_of(distribution):
    """The mean of one ``['normal', loc, scale]`` / ``['exponential', scale]`` / ``['uniform', loc, scale]`` entry."""
    kind = distribution[0]
    if kind == "normal":
        return float(distribution[1])
    if kind == "exponential":
        return float(distribution[1])
    if kind == "uniform":
        return float(distribution[1]) + 0.5 * float(distribution[2])
    raise NotImplementedError(f"mean_of: distribution {kind!r}")


def routing_matrix(sim_matrix):
    """(dim, dim) routing probabilities of a spec's ``sim_matrix`` as the SIMULATOR routes: row i's positive off-diagonal
    flows over their sum -- and, where those quotients do not add up to exactly 1.0 in floating point, uniform over
    the children (the reference then calls ``np.random.choice(children)`` without p).  A childless row is zero."""
    adj = np.asarray(sim_matrix, dtype=np.float64)
    dim = adj.shape[0]
    p = np.zeros((dim, dim))
    for i in range(dim):
        ch = [j for j in range(dim) if j != i and adj[i, j] > 0]
        if not ch:
            continue
        flows = [float(adj[i, j]) for j in ch]
        q = [f / sum(flows) for f in flows]
        if sum(q) != 1:
            q = [1.0 / len(ch)] * len(ch)
        p[i, ch] = q
    return p


def traffic_rates(spec):
    """Arrival rate at every node of an open net without blocking: lam = lam0 + lam P on the servers' rows of
    ``routing_matrix``, lam0[j] = sum over sources s of P[s, j] / (mean inter-arrival time of s).  -> (dim) float64:
    a server's total arrival rate, a source's own rate.  Raises ValueError when (I - P^T) is singular (customers that
    never leave: a closed loop)."""
    adj = np.asarray(spec.sim_matrix, dtype=np.float64)
    dim = adj.shape[0]
    p = routing_matrix(adj)
    source = np.diagonal(adj) > 0
    rate = np.zeros(dim)
    for s in np.flatnonzero(source):
        m = mean_of(spec.distributions[s])
        if not m > 0:
            raise ValueError(f"traffic_rates: source {s} has mean inter-arrival time {m}")
        rate[s] = 1.0 / m
    servers = np.flatnonzero(~source)
    lam0 = rate[source] @ p[source][:, servers]
    a = np.eye(len(servers)) - p[np.ix_(servers, servers)].T
    if len(servers) and np.linalg.matrix_rank(a) < len(servers):
        raise ValueError("traffic_rates: (I - P^T) is singular: some customers never leave the net")
    out = rate.copy()
    if len(servers):
        out[servers] = np.linalg.solve(a, lam0)
    return out
