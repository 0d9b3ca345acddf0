"""The table of cases of tests/test_col_groups_cpu.py: the jobs of the five launchers that take their workgroups from the
column-group geometry of csrc/mpdata_wm_walk.h (col_groups_batched: column_path, vsolve, column_step; col_groups_tiled:
sediment, cell_add without and with dsum), as rows of integers
    call ipe slp nlev nx ntr ncrms W nz sl0 n
in the order tests/stubs/col_groups_probe.cpp reads them.  tests/golden/col_groups_parent.npz holds this table and what
the launchers computed for it BEFORE the geometry was shared (docs/EXPERIMENTS.md Z).
"""
CALLS = ("cp", "vs", "cs", "sed", "cad", "cadsum")
NX = (1, 2, 3, 8, 9, 32, 33, 64, 200)
TALL = (239, 250, 300, 1000)
FIELDS = ("UG", "CB", "ns", "g0", "ngroup", "lds", "ncb", "nround", "ush")


def plan_side(nz):
    """(slp, nlev, W) of the plan mpdata_plan_create makes for nz levels (mpdata_plan.hip: slp = 64 / LPS, one above 32
    levels; mpdata_windows.h: the inner plan of a windowed one)"""
    if nz <= 238:
        return (8 if nz <= 8 else 4 if nz <= 16 else 2 if nz <= 32 else 1), nz - 1, 1
    nzm = nz - 1
    W = (nzm - 6 + 56) // 57
    return 1, (nzm + 6 * (W - 1) + W - 1) // W, W


def blocks(ncrms, gi):
    """six blocks of a plan whose widest group holds gi instances: the whole plan, the first and the last instance alone,
    ends inside groups, a start at a group boundary, and a start inside a group up to the last instance (on an odd fp32
    plan the partner of the phantom)"""
    return ((0, ncrms), (0, 1), (ncrms - 1, 1), (3, gi + 4), (gi, gi // 2 + 1), (gi + 1, ncrms - gi - 1))


def plan_cases():
    for nz in list(range(2, 239)) + list(TALL):
        slp, nlev, W = plan_side(nz)
        for ipe in (1, 2):
            gi = ipe * max(16, 4 * slp)         # instances of the widest group; narrower ones divide it
            ncrms = 2 * gi + 5 * ipe - (ipe == 2)   # two groups and a part of a third; fp32: odd, the last pair half phantom
            ntr = 1 + nz % 3
            for nx in NX:
                for sl0, n in blocks(ncrms, gi):
                    for call in range(len(CALLS)):
                        if CALLS[call] == "cs" and W > 1:   # (refused before the geometry: mpdata_column_step_wm)
                            continue
                        yield (call, ipe, slp, nlev, nx, ntr, ncrms, W, nz, sl0, n)


def guard_cases():
    """jobs no plan makes: one refused case, at least, per guard that can be reached behind wm_block_grid"""
    cp, vs, cs, sed, cad, cadsum = range(6)
    out = []
    for call in (cp, vs, cs):
        out.append((call, 1, 3, 20, 8, 1, 40, 1, 21, 0, 40))           # UG is no multiple of slp
        out.append((call, 1, 1, 6000, 8, 1, 40, 1, 6001, 0, 40))       # one column and the rows do not fit at UG = slp
        out.append((call, 1, 128, 1, 8, 1, 600, 1, 2, 0, 600))         # UG = 512 > 256
        # groups x tracers x batches beyond an int (the grid of wm_block_grid still fits)
        out.append((call, 1, 1, 20, 200, 8000, 1 << 20, 1, 21, 0, 1 << 20))
    for call in (vs, cs, sed, cad, cadsum):
        out.append((call, 1, 12, 5, 8, 1, 100, 1, 6, 0, 100))          # UG = 48: no power of two (column_path divided)
    # units beyond an int: the last instance of 2^31 + 8 at eight per tile.  column_path counts in long long and runs it.
    for call in range(6):
        out.append((call, 1, 8, 7, 8, 1, (1 << 31) + 8, 1, 8, (1 << 31) + 7, 1))
    # ... times W in vsolve: the last instance of an fp32 plan of 18 windows whose tiles just fit an int
    for call in (cp, vs, sed, cad, cadsum):
        out.append((call, 2, 1, 62, 8, 1, 238609294, 18, 1000, 238609293, 1))
    out.append((vs, 1, 1, 40, 8, 1, 4, 200, 7000, 0, 4))               # vsolve: a window table beyond its 128 threads
    for call in (sed, cad, cadsum):
        out.append((call, 1, 1, 300, 8, 1, 40, 1, 301, 0, 40))         # five slices: a tile is more than a workgroup's
        out.append((call, 1, 1, 60, 8, 1, 1, 70000, 4000000, 0, 1))    # W beyond gridDim.y
        out.append((call, 2, 256, 1, 8, 1, 2000, 1, 2, 0, 2000))       # more instances in a group than lanes
    return out


def cases():
    return list(plan_cases()) + guard_cases()


def line(c):
    return " ".join([CALLS[c[0]]] + [str(x) for x in c[1:]])


def parse(out):
    """the probe's output -> one row per case: (1, fields ...) or (0, zeros); a field the call does not have is -1"""
    rows = []
    for ln in out.splitlines():
        res = ln.split("->")[1].split()
        if res == ["refuse"]:
            rows.append([0] * (1 + len(FIELDS)))
            continue
        d = dict(zip(res[0::2], res[1::2]))
        rows.append([1] + [int(d.get(k, -1)) for k in FIELDS])
    return rows
