// col_groups_probe.cpp -- the column-group geometry of csrc/mpdata_wm_walk.h over a table of cases, on the host alone
// (tests/test_col_groups_cpu.py builds and runs it; no device is touched).
//   stdin: one case per line, `call ipe slp nlev nx ntr ncrms W nz sl0 n`; '#' starts a comment.
//     call: cp, vs, cs, sed, cad, cadsum -- the five launchers (cell-add without and with dsum); the rest is the plan
//     side as mpdata_plan_create and wm_job make it: ipe reals per 8-byte element, slp elements per tile, nlev levels of a
//     chunk (of a window in a windowed plan: W > 1, nz the tall column), nx interior columns, ntr tracers of the call,
//     ncrms instances of the plan, the block [sl0, sl0 + n).
//   stdout: the case and `refuse`, or every field the launcher takes from the geometry.
#include <cstdio>
#include <cstring>

#include "mpdata_wm_walk.h"

using namespace wm_walk;

int main() {
  char line[512], call[16];
  static double f[1];
  while (fgets(line, sizeof line, stdin)) {
    long long ncrms, sl0, n;
    int ipe, slp, nlev, nx, ntr, W, nz;
    if (line[0] == '#' || sscanf(line, "%15s %d %d %d %d %d %lld %d %d %lld %lld", call, &ipe, &slp, &nlev, &nx, &ntr, &ncrms, &W, &nz, &sl0,
                                 &n) != 11)
      continue;
    MpdataLayoutJob j;
    memset(&j, 0, sizeof j);
    const long long elems = (ncrms * W + ipe - 1) / ipe;
    j.prv = f; j.ncrms = elems; j.nlev = nlev; j.ntr = ntr; j.slp = slp;
    j.ntiles = (int)((elems + slp - 1) / slp);
    j.ncol_p = nx + 6; j.ncols = j.ncol_p; j.prv_col0 = 0;
    j.chunk = (long long)slp * nlev;
    j.main_e = j.chunk / 16 * 16;
    long long lines = ((long long)j.ncol_p * j.chunk * 8 + 127) / 128;
    lines += (lines & 1) == 0;
    j.prv_tile_stride = lines * 16;
    j.prv_tstride = j.prv_tile_stride * j.ntiles;
    MpdataBlockSel b;
    b.sl0 = sl0; b.n = n; b.ncrms = ncrms; b.ipe = ipe; b.W = W; b.nz = nz;
    line[strcspn(line, "\n")] = 0;
    printf("%s ->", line);
    WmGrid wg;
    ColGroups g;
    bool ok = wm_block_grid(j, b, ntr, &wg) == hipSuccess, batched = true;
    // the arguments of the five launchers, as they pass them
    if (!ok) {
    } else if (!strcmp(call, "cp")) {
      ok = col_groups_batched(j, b, wg, 4096, 0, 1, 0, &g);
    } else if (!strcmp(call, "vs")) {
      ok = W <= 128 && (W == 1 || j.chunk <= 64) && col_groups_batched(j, b, wg, LDS_ELEMS, W > 1 ? 2 * W * ipe : 0, 3, W, &g);
    } else if (!strcmp(call, "cs")) {
      ok = W == 1 && col_groups_batched(j, b, wg, LDS_ELEMS, 9, 0, 1, &g);
    } else {
      batched = false;
      if (!strcmp(call, "sed")) ok = col_groups_tiled(j, b, wg, LDS_ELEMS, W > 1 ? 4 : 0, 1, 1, true, true, &g);
      else if (!strcmp(call, "cad")) ok = col_groups_tiled(j, b, wg, LDS_ELEMS, W > 1 ? 4 : 0, 0, 2, false, false, &g);
      else if (!strcmp(call, "cadsum")) ok = col_groups_tiled(j, b, wg, LDS_ELEMS, W > 1 ? 4 : 0, 0, 2, true, false, &g);
      else ok = false;
    }
    if (!ok) {
      printf(" refuse\n");
      continue;
    }
    printf(" UG %d CB %d ns %d g0 %lld ngroup %lld lds %lld", g.UG, g.CB, g.ns, g.g0, g.ngroup, g.lds_e * 8);
    if (batched) printf(" ncb %d", g.ncb);
    else printf(" nround %d", g.nround);
    if (strcmp(call, "cp")) printf(" ush %d", g.ush);   // (column_path divides)
    printf("\n");
  }
  return 0;
}
