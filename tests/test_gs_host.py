"""The multicolour Gauss-Seidel smoother of the aggregation V-cycle (MgSetSmoother(mg, 1)) on the host side, no GPU needed: the numpy
yardstick of tests/test_gpu_gs.py lives here.

``GsHierarchy`` is ``Hierarchy`` of tests/test_amg_host.py with the colouring and the cycle of include/MgcgGpu.h (MgSetSmoother) stated in
np.float64 and 32-bit unsigned integers: the colouring round by round, a sweep colour by colour in place with every row summed serially in
stored order (``row_sums``), forward sweeps before the coarse correction, backward sweeps after it, alternating sweeps on the last level.
The HIP colouring and cycle must EQUAL it.

Iterations of the yardstick PCG loop to a relative 1e-8, N(0,1) right-hand side (seed 1), every sum of the loop a serial sum
(``serial_dot``), three levels, measured here:

    system                          Jacobi V-cycle (omega 0.8)   Gauss-Seidel V-cycle (omega 1)   one level, forward + backward sweep
    permuted(poisson 12^3, 7)                  17                           13                               23
    graph_laplacian(10, 7)                     50                           40                               96

``test_gs_cuts_the_iterations_of_the_jacobi_cycle`` prints the three counts and asserts GS <= Jacobi on these two systems."""
import ctypes as C

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from tests.test_amg_host import (Hierarchy, arrowhead, csr_of, dominant_graph, graph_laplacian, irregular_maps, one_way, permuted, rows_per_level, serial_dot,
                                 with_duplicates)
from tests.test_mixed_host import row_sums

U32 = np.uint64(0xFFFFFFFF)
MAX_COLOURS = 64


# --------------------------------------------------------------------------- the yardstick: colouring
def row_key(i):
    """The key of the rows i (array), 32-bit unsigned arithmetic carried in uint64 and masked."""
    h = (np.asarray(i, dtype=np.uint64) * np.uint64(0x9E3779B1)) & U32
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & U32
    h ^= h >> np.uint64(12)
    h = (h * np.uint64(0x297A2D39)) & U32
    h ^= h >> np.uint64(15)
    return h


def colouring(c, ro):
    """(colour of every row, rounds): the rounds of the header.  ValueError("row i") for the smallest row of a round whose coloured
    neighbours hold all 64 colours, and -- after the rounds -- for the smallest row that stores an entry of a row of its own colour."""
    n = len(ro) - 1
    rows = np.repeat(np.arange(n), np.diff(ro))
    c = np.asarray(c, dtype=np.int64)
    off = c != rows
    ri, cj = rows[off], c[off]
    h = row_key(np.arange(n))
    larger = (h[cj] > h[ri]) | ((h[cj] == h[ri]) & (cj > ri))          # the neighbour compares larger than the row
    colour = np.full(n, -1, dtype=np.int64)
    rounds = 0
    while (colour < 0).any():
        open_ = colour < 0
        beaten = np.zeros(n, dtype=bool)
        beaten[ri[open_[ri] & open_[cj] & larger]] = True
        winners = open_ & ~beaten
        held = np.zeros(n, dtype=np.uint64)
        seen = winners[ri] & ~open_[cj]
        np.bitwise_or.at(held, ri[seen], np.uint64(1) << colour[cj[seen]].astype(np.uint64))
        w = np.nonzero(winners)[0]
        free = ~held[w]
        if (free == 0).any():
            raise ValueError(f"row {int(w[free == 0].min())}")
        lowest = free & (np.uint64(0) - free)                         # the lowest set bit: a power of two, exact as a double
        colour[w] = np.log2(lowest.astype(np.float64)).astype(np.int64)
        rounds += 1
    same = colour[ri] == colour[cj]
    if same.any():
        raise ValueError(f"row {int(ri[same].min())}")
    return colour.astype(np.int32), rounds


def colour_lists(e, c, ro, colour):
    """Per colour: (rows ascending, the CSR of those rows alone)."""
    out = []
    ro = np.asarray(ro, dtype=np.int64)
    for q in range(int(colour.max()) + 1 if len(colour) else 0):
        rows = np.nonzero(colour == q)[0]
        length = (ro[1:] - ro[:-1])[rows]
        first = np.cumsum(length) - length
        k = np.repeat(ro[rows] - first, length) + np.arange(int(length.sum()))
        out.append((rows, e[k], c[k], np.r_[0, np.cumsum(length)]))
    return out


class GsHierarchy(Hierarchy):
    """Hierarchy with the multicolour Gauss-Seidel cycle; ValueError("level l, row i") where MgSetSmoother refuses a level."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.rounds = []
        for l, L in enumerate(self.levels):
            try:
                L["colour"], rounds = colouring(L["c"], L["ro"])
            except ValueError as err:
                raise ValueError(f"level {l}, {err}") from None
            self.rounds.append(rounds)
            L["lists"] = colour_lists(L["e"], L["c"], L["ro"], L["colour"])

    def colours(self):
        return [len(L["lists"]) for L in self.levels]

    def _sweep(self, L, b, x, forward):
        for rows, e, c, ro in (L["lists"] if forward else L["lists"][::-1]):
            res = b[rows] - row_sums(e, c, ro, x)
            t = L["dinv"][rows] * res
            step = self.omega * t
            x[rows] = x[rows] + step

    def _vcycle(self, l, b):
        L = self.levels[l]
        x = np.zeros(len(b))
        if l == len(self.levels) - 1:
            for s in range(self.nuCoarse):
                self._sweep(L, b, x, s % 2 == 0)
            return x
        for _ in range(self.nu):
            self._sweep(L, b, x, True)
        r = b - row_sums(L["e"], L["c"], L["ro"], x)
        members = np.argsort(L["map"], kind="stable")
        offsets = np.r_[0, np.cumsum(np.bincount(L["map"], minlength=L["nc"]))]
        bc = row_sums(np.ones(len(members)), members, offsets, r)
        ec = self._vcycle(l + 1, bc)
        x = x + ec[L["map"]]
        for _ in range(self.nu):
            self._sweep(L, b, x, False)
        return x


def banded(n, half, seed=4):
    """n rows coupled to the `half` rows either side with weights U(0.5, 2), diagonal 1.25 x the off-diagonal row sum: 2 half + 1 entries
    a row away from the ends and half + 1 colours at least (rows i .. i + half all see each other)."""
    import scipy.sparse as sp

    from tests.test_amg_host import system_of

    rng = np.random.default_rng(seed)
    bands = [rng.uniform(0.5, 2.0, n - k) for k in range(1, half + 1)]
    W = sp.diags(bands + bands, list(range(1, half + 1)) + [-k for k in range(1, half + 1)]).tocsr()
    return system_of(sp.diags(1.25 * np.asarray(W.sum(axis=1)).ravel()) - W, f"banded-{n}-{half}")


# --------------------------------------------------------------------------- the colouring
SYSTEMS = {
    "poisson12-permuted": lambda: permuted(problems.poisson(12, 12, 12), 7),
    "graph10": lambda: graph_laplacian(10, 3),
    "arrowhead": arrowhead,
    "duplicates": lambda: with_duplicates(graph_laplacian(8, 3)),
    "banded-12": lambda: banded(300, 12),
}


def test_row_key_is_32_bit_and_the_header_formula():
    i = np.array([0, 1, 5, 70000, 2 ** 31 - 1])
    h = row_key(i)
    assert h.max() <= 0xFFFFFFFF
    k = (5 * 0x9E3779B1) & 0xFFFFFFFF                           # one key by hand, Python integers
    k ^= k >> 15
    k = (k * 0x2C1B3C6D) & 0xFFFFFFFF
    k ^= k >> 12
    k = (k * 0x297A2D39) & 0xFFFFFFFF
    k ^= k >> 15
    assert int(h[2]) == k and int(h[0]) == 0


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_every_colouring_is_proper_within_64_colours_and_reproducible(name):
    s = SYSTEMS[name]()
    H = GsHierarchy(*csr_of(s))
    print(f"{name}: rows per level {rows_per_level(H)}, colours {H.colours()}, rounds {H.rounds}")
    for L in H.levels:
        n = len(L["ro"]) - 1
        colour = L["colour"]
        assert len(colour) == n and colour.min() == 0 and colour.max() < MAX_COLOURS
        rows = np.repeat(np.arange(n), np.diff(L["ro"]))
        off = L["c"] != rows
        assert np.all(colour[rows[off]] != colour[L["c"][off]])                              # proper
        assert np.array_equal(np.unique(colour), np.arange(colour.max() + 1))                # no colour skipped: the smallest free one is taken
        # every row of colour q > 0 sees every colour below q (it took the smallest free one)
        below = np.zeros(n, dtype=np.uint64)
        np.bitwise_or.at(below, rows[off], np.uint64(1) << colour[L["c"][off]].astype(np.uint64))
        want = (np.uint64(1) << colour.astype(np.uint64)) - np.uint64(1)
        assert np.all(below & want == want)
        assert np.array_equal(np.sort(np.concatenate([rows_ for rows_, _, _, _ in L["lists"]])), np.arange(n))
        assert all(np.all(np.diff(rows_) > 0) for rows_, _, _, _ in L["lists"])
    again = GsHierarchy(*csr_of(SYSTEMS[name]()))
    assert all(np.array_equal(L["colour"], K["colour"]) for L, K in zip(H.levels, again.levels))


def test_colouring_by_hand_on_a_path_of_four_rows():
    ro, c = np.array([0, 2, 5, 8, 10]), np.array([0, 1, 0, 1, 2, 1, 2, 3, 2, 3])
    h = [int(v) for v in row_key(np.arange(4))]
    colour = [-1] * 4
    rounds = 0
    while min(colour) < 0:                                       # the rule in plain Python
        start = list(colour)
        for i in range(4):
            nb = [j for j in (i - 1, i + 1) if 0 <= j < 4]
            if start[i] < 0 and all((h[i], i) > (h[j], j) for j in nb if start[j] < 0):
                colour[i] = min(q for q in range(64) if q not in [start[j] for j in nb])
        rounds += 1
    got, got_rounds = colouring(c, ro)
    assert got.tolist() == colour and got_rounds == rounds


def test_the_yardstick_refuses_what_the_library_refuses():
    # an entry without a mirror: two rows that do not both see each other may take one colour -- the check names the row
    s = one_way(graph_laplacian(10, 3))
    with pytest.raises(ValueError, match=r"^level 0, row \d+$"):
        GsHierarchy(*csr_of(s))
    # a band of 70 rows either side: rows i .. i + 70 all see each other, 71 colours at least
    with pytest.raises(ValueError, match=r"^level 0, row \d+$"):
        GsHierarchy(*csr_of(banded(200, 70)), maps=[])
    # the dense band of the reference's main(): the same refusal at a few hundred rows
    with pytest.raises(ValueError, match=r"^level 0, row \d+$"):
        GsHierarchy(*csr_of(problems.viennacl_main(n=300)), maps=[])


def test_irregular_maps_stay_within_64_colours():
    s = dominant_graph(10, 3)
    H = GsHierarchy(*csr_of(s), maps=irregular_maps(s.Count))
    print("irregular: rows per level", rows_per_level(H), "colours", H.colours())
    assert max(H.colours()) <= MAX_COLOURS and H.colours()[-1] == 1


# --------------------------------------------------------------------------- the cycle
def _asymmetry(H, n, seed=9):
    rng = np.random.default_rng(seed)
    u, v = rng.standard_normal(n), rng.standard_normal(n)
    a, b = float(u @ H.apply(v)), float(v @ H.apply(u))
    return abs(a - b) / abs(a)


@pytest.mark.parametrize("levels", [1, 3])
def test_the_cycle_is_symmetric_for_an_even_coarse_count_only(levels):
    """<u, M^-1 v> = <v, M^-1 u> to rounding when the last level runs an even number of alternating sweeps; a single forward sweep there
    is (D/omega + L)^-1, not a symmetric operator, and the cycle around it is not one either: what MgSetSmoother's refusal is for."""
    s = permuted(problems.poisson(12, 12, 12), 7)
    maps = dict(maps=[]) if levels == 1 else dict(levels=3)
    for nuc in (2, 4):
        for omega in (1.0, 1.5):
            d = _asymmetry(GsHierarchy(*csr_of(s), omega=omega, nuCoarse=nuc, **maps), s.Count)
            print(f"levels {levels} nuCoarse {nuc} omega {omega}: |a - b| / |a| = {d:.2e}")
            assert d <= 1e-12
    d = _asymmetry(GsHierarchy(*csr_of(s), omega=1.0, nuCoarse=1, **maps), s.Count)
    print(f"levels {levels} nuCoarse 1: |a - b| / |a| = {d:.2e}")
    assert d > 1e-6


def test_one_sweep_from_zero_is_the_jacobi_first_sweep_on_the_first_colour():
    s = graph_laplacian(6, 2)
    H = GsHierarchy(*csr_of(s), maps=[], nuCoarse=2)
    L = H.levels[0]
    b = np.random.default_rng(3).standard_normal(s.Count)
    x = np.zeros(s.Count)
    H._sweep(L, b, x, True)
    first = L["lists"][0][0]
    assert np.array_equal(x[first], (H.omega * (L["dinv"] * b))[first])
    # ... and a forward sweep solves (D / omega + L) x = b in the colour order: every row's residual vanishes against the rows before it
    order = np.concatenate([rows for rows, _, _, _ in L["lists"]])
    A = s.to_scipy().toarray()[order][:, order]
    lower = np.tril(A, -1) + np.diag(np.diag(A)) / H.omega
    assert np.abs(lower @ x[order] - b[order]).max() <= 1e-12 * np.abs(b).max() * np.abs(A).max()


def _iterations(H, s):
    out = H.pcg(np.asarray(s.b), tol=1e-8 * float(np.linalg.norm(s.b)), dot=serial_dot)
    assert out["status"] == _lib.OK
    assert np.linalg.norm(s.b - s.to_scipy() @ out["x"]) < 2e-8 * float(np.linalg.norm(s.b))
    return out["iteration"]


@pytest.mark.parametrize("name", ["poisson12-permuted", "graph10-7"])
def test_gs_cuts_the_iterations_of_the_jacobi_cycle(name):
    s = permuted(problems.poisson(12, 12, 12), 7) if name == "poisson12-permuted" else graph_laplacian(10, 7)
    s.b = np.random.default_rng(1).standard_normal(s.Count)
    e, c, ro = csr_of(s)
    jacobi = _iterations(Hierarchy(e, c, ro, levels=3, omega=0.8), s)
    G = GsHierarchy(e, c, ro, levels=3, omega=1.0)
    gs = _iterations(G, s)
    ssor = _iterations(GsHierarchy(e, c, ro, maps=[], omega=1.0, nuCoarse=2), s)
    print(f"{name}: rows per level {rows_per_level(G)}, colours {G.colours()}, rounds {G.rounds}; iterations: Jacobi V-cycle {jacobi}, GS V-cycle {gs}, one level F+B {ssor}")
    assert len(G.levels) == 3
    assert gs <= jacobi


# --------------------------------------------------------------------------- the library without a device
def test_exports_and_python_surface(hiplib):
    for name in ("MgSetSmoother", "MgSmoother", "MgLevelColours", "MgLevelCopyColours"):
        assert hasattr(hiplib, name) and name in _lib.SIGNATURES
    assert hiplib.MgcgAbiVersion() == 3
    import conjugategradient_amd
    from conjugategradient_amd import amg, ssor

    assert "ssor" in conjugategradient_amd.__all__
    assert issubclass(ssor.ConjugateGradientSsorGpu, amg.ConjugateGradientAmgGpu)
    assert callable(amg.ConjugateGradientAmgGpu.level_colours)
    for member in ("Apply", "Solve", "SolveMinres", "SolveBicgstab"):
        assert callable(getattr(ssor.ConjugateGradientSsorGpu, member))
    with pytest.raises(_lib.MgcgError, match="smoother 'sor'"):
        amg.ConjugateGradientAmgGpu(10, 3, 0, 10, 1e-8, smoother="sor")


def test_bad_arguments_are_refused_with_a_message_before_any_device_call(hiplib):
    L = hiplib
    handle = C.create_string_buffer(4096)                      # stands for the hierarchy: a refused call does not look at it
    h = C.addressof(handle)
    out = np.zeros(4, dtype=np.int32)

    def message(call):
        L.MgcgClearLastError()
        status = call()
        msg = _lib.last_error()
        L.MgcgClearLastError()
        return status, msg

    for mode in (0, 1):
        status, msg = message(lambda: L.MgSetSmoother(None, mode))
        assert status == -1 and "MgSetSmoother: null handle" in msg
    for mode in (-1, 2, 7):
        status, msg = message(lambda: L.MgSetSmoother(h, mode))
        assert status == -1 and f"MgSetSmoother: mode {mode}, must be 0" in msg, msg
    assert L.MgSmoother(None) == 0
    status, msg = message(lambda: L.MgLevelColours(None, 0))
    assert status == -1 and "MgLevelColours" in msg
    status, msg = message(lambda: L.MgLevelCopyColours(None, 0, out.ctypes.data))
    assert status == -1 and "MgLevelCopyColours: null argument" in msg
    status, msg = message(lambda: L.MgLevelCopyColours(h, 0, None))
    assert status == -1 and "MgLevelCopyColours: null argument" in msg
