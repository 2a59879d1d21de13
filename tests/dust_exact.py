"""An independent statement of vsearch's DUST soft mask, in plain Python (no test functions): what the clustering and the
orientation models (tests/test_cluster_cpu.py, tests/cluster_edges.py, tests/orient_exact.py) mask their seeds with, and what
the oracle's orc_dust, the engine's k_dust and the engine's host statement dust_host are each held to."""


def py_dust(seq):
    """vsearch's DUST soft mask (mask.cc dust()/wo(), after Tatusov & Lipman), stated independently of orc_dust: windows of 64
    that advance by 32, 3-mer repeat score 10 * sum / j, masked above 20, the first best interval in (i, j) order"""
    code = {"A": 0, "C": 1, "G": 2, "T": 3, "U": 3}
    s = [code.get(c, 0) for c in seq.upper()]
    masked = [False] * len(s)
    i = 0
    while i < len(s):
        win = s[i:i + 64]
        n = len(win)
        best = (0, 0, 0)
        if n - 7 >= 0:
            tri = [((win[j - 2] if j >= 2 else 0) << 4 | (win[j - 1] if j >= 1 else 0) << 2 | win[j]) for j in range(n)]
            for a in range(n - 7):
                seen, total = {}, 0
                for j in range(2, n - a):
                    w = tri[a + j]
                    c = seen.get(w, 0)
                    if c:
                        total += c
                        v = 10 * total // j
                        if v > best[0]:
                            best = (v, a, j)
                    seen[w] = c + 1
        v, a, j = best
        if v > 20:
            for k in range(a + i, a + j + i + 1):
                masked[k] = True
            if a + j < 32:
                i += 32 - (a + j)
        i += 32
    return masked
