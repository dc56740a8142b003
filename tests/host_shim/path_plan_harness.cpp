// Compiles csrc/path_plan.h for the host (test infrastructure; tests/test_path_plan_host.py): (a) pinned rows — the plan and the
// to_solver_path report of named configurations at 256 compute units, derived by hand from the to_create / to_solver_path that held this
// logic before it moved into path_plan.h; (b) invariants over a sweep of every model's traits x batch sizes x constraints x cost blocks x
// every knob at its extreme values; (c) counts of what was reached.  The knobs go through read_path_knobs with a table as environment.
#include "path_plan.h"

#include <cstdio>
#include <map>
#include <string>
#include <vector>
using namespace to;

static long long fails = 0, checks = 0;
#define CHECK(c, ...) do { ++checks; if (!(c)) { if (fails < 30) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++fails; } } while (0)

static std::map<std::string, std::string> g_env;
static const char* lookup(const char* name) { auto it = g_env.find(name); return it == g_env.end() ? nullptr : it->second.c_str(); }
static PathKnobs knobs(const char* env) {  // "NAME=value NAME=value" (names without the TRAJOPT_ prefix)
  g_env.clear();
  std::string s = env ? env : "";
  for (size_t i = 0; i < s.size();) {
    const size_t e = s.find('=', i), sp = s.find(' ', e) == std::string::npos ? s.size() : s.find(' ', e);
    g_env["TRAJOPT_" + s.substr(i, e - i)] = s.substr(e + 1, sp - e - 1);
    i = sp + 1;
  }
  return read_path_knobs(lookup);
}

// ---- the trait sets of models.h, with the optional launchers the ops_*.hip translation units fill -----------------------------
struct Model { const char* name; int ne, m; PathTraits t; };
static PathTraits traits(bool wt, bool mfma, bool coop, bool lane, int ls, bool eb, bool ebc, bool ebs, bool ar, bool elk, bool ec, uint32_t f, uint32_t f2, uint32_t fp) {
  PathTraits t;
  t.write_through = wt; t.mfma_backward = mfma; t.coop_backward = coop; t.lane_backward = lane; t.ls_first_round = ls;
  t.expand_backward = eb; t.expand_backward_coop = ebc; t.expand_backward_scan = ebs; t.accept_roll = ar; t.expand_lane_k = elk; t.expand_const = ec;
  t.forward = f; t.forward2 = f2; t.forward_plants = fp;
  return t;
}
constexpr uint32_t F_SMALL = 0xFFFFu;  // variants 0..15 (models that pin RK4)
constexpr uint32_t F_QUAD = 0x0F0Fu | (3u << 18) | (3u << 26);  // 0-3, 8-11, 18-19, 26-27
constexpr uint32_t F_ATT = (1u << 8) | (1u << 10);
// one plant per trajectory: the general variants (bit 3) of the models to_set_model_params_batch accepts; 12 / 14 where RK4 is pinned
constexpr uint32_t FP_SMALL = (1u << 8) | (1u << 10) | (1u << 12) | (1u << 14), FP_QUAD = (1u << 8) | (1u << 10);
static const Model MODELS[] = {
    {"double integrator 1", 2, 1, traits(true, false, true, true, 4, true, true, true, true, true, false, F_SMALL, F_SMALL, FP_SMALL)},
    {"double integrator 2", 4, 2, traits(true, false, true, true, 4, true, true, true, true, true, false, F_SMALL, F_SMALL, FP_SMALL)},
    {"double integrator 3", 6, 3, traits(true, false, true, false, 4, false, false, false, true, false, false, F_SMALL, F_SMALL, FP_SMALL)},
    {"cartpole", 4, 1, traits(true, true, true, true, 4, true, true, true, true, true, false, F_SMALL, F_SMALL, FP_SMALL)},
    {"quadrotor", 12, 4, traits(false, true, false, false, 16, false, false, false, true, false, true, F_QUAD, F_QUAD, FP_QUAD)},
    {"quadrotor mrp/rp", 12, 4, traits(false, true, false, false, 16, false, false, false, true, false, true, F_ATT, F_ATT, 0u)},
    {"hybrid", 4, 2, traits(true, false, true, true, 4, true, true, true, true, true, false, F_SMALL, F_SMALL, 0u)},
    {"model vector", 6, 3, traits(true, false, true, false, 4, false, false, false, true, false, false, F_SMALL, F_SMALL, 0u)},
    {"infeasible di 1", 2, 3, traits(true, false, true, false, 4, false, false, false, true, false, false, F_SMALL, F_SMALL, 0u)},
    {"infeasible di 2", 4, 6, traits(true, false, true, false, 4, false, false, false, true, false, false, F_SMALL, F_SMALL, 0u)},
    {"infeasible cartpole", 4, 5, traits(true, false, true, false, 4, false, false, false, true, false, false, F_SMALL, F_SMALL, 0u)},
};
enum { DI1, DI2, DI3, CART, QUAD, QATT, HYB, VEC, INF1, INF2, INFC, N_MODELS };

static PathShape shape(const Model& M, int B, int N, int n_cons, bool diag, int ls = 20, int cus = 256) {
  PathShape s;
  s.B = B; s.Bp = (B + 63) / 64 * 64; s.N = N; s.ne = M.ne; s.m = M.m; s.n_cons = n_cons; s.iterations_linesearch = ls; s.diagonal_cost_blocks = diag; s.cus = cus;
  return s;
}
// KArgs::h_diag as upload_tables derives it
static int h_diag_of(const PathPlan& p, bool diag, bool full_blocks = false) { return (!p.bwd_mfma && !p.bwd_lane && diag && !full_blocks) ? 1 : 0; }

static std::string plan_text(const PathPlan& p) {
  char b[512];
  snprintf(b, sizeof b, "bwd=%d fc=%d fl=%d scan=%d/%d cmp=%d fwd2=%d mrg=%d pack=%d elane=%d cw=%d/%d deep=%d/%d/%d roll=%d/%g rp=%d/%g ls2=%d/%d/%d/%d waves=%lld dump=%d rb0=%d xb=%lld ub=%lld",
           p.bwd_mfma ? 1 : p.bwd_lane ? 2 : 0, p.fused_coop, p.fused_lane, p.scan, p.scan_max_active, p.compact, p.fwd2, p.coop_merge, p.expand_pack, p.expand_lane,
           p.cw_base, p.tw_base, p.cw_deep, p.tw_deep, p.deep_max_active, p.roll_min_active, p.roll_min_frac, p.rp_min, p.rp_at,
           p.ls2_cwa, p.ls2_cwb, p.ls2_blkA, p.ls2_dump, p.waves, p.dump_wave, p.repack_block0, p.x_blocks, p.u_blocks);
  return b;
}

// ---- (a) pinned rows ---------------------------------------------------------------------------------------------------------------
// info: what to_solver_path reports; plan: scan=S/max, roll=min/frac, rp=min/at, ls2=cwa/cwb/blkA/dump.  Both worked out by hand from the code
// that selected the path inside to_create before path_plan.h existed (tests/test_gpu_parity.py::test_solver_path_of_created_handles asks a
// built library for some of these rows).  expand_variant: 0 diagonal-kind costs without constraints, 2 with selector constraints, 6 with
// generic ones.
struct Row { const char* name; int model, B, N, n_cons; bool diag; int ev, ls; const char* env; int info[8]; const char* plan; };
static const Row ROWS[] = {
    {"C2 cartpole B1024 N101", CART, 1024, 101, 0, true, 0, 20, "", {0, 1, 0, 4, 2, 1, 1, 0},
     "bwd=0 fc=1 fl=0 scan=1/1073741824 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=64 dump=64 rb0=0 xb=65 ub=65"},
    {"cartpole B1024 N11", CART, 1024, 11, 0, true, 0, 20, "", {0, 1, 0, 4, 2, 1, 1, 0},
     "bwd=0 fc=1 fl=0 scan=1/1073741824 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=64 dump=64 rb0=0 xb=65 ub=65"},
    {"quadrotor B4096 N11", QUAD, 4096, 11, 0, false, 0, 20, "", {1, 0, 1, 16, 2, 0, 1, 1},
     "bwd=1 fc=0 fl=0 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=16/4 deep=20/3/3072 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=1366 dump=1366 rb0=1367 xb=2733 ub=2733"},
    {"C3 quadrotor B4096 N201", QUAD, 4096, 201, 0, false, 0, 20, "", {1, 0, 1, 16, 2, 0, 1, 1},
     "bwd=1 fc=0 fl=0 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=16/4 deep=20/3/3072 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=1366 dump=1366 rb0=1367 xb=2733 ub=2733"},
    {"quadrotor B4096 N101 ls20", QUAD, 4096, 101, 0, false, 0, 20, "", {1, 0, 1, 16, 2, 0, 1, 1},
     "bwd=1 fc=0 fl=0 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=16/4 deep=20/3/3072 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=1366 dump=1366 rb0=1367 xb=2733 ub=2733"},
    {"C5 quadrotor AL B8192 N201", QUAD, 8192, 201, 2, false, 2, 20, "", {1, 0, 1, 8, 2, 0, 1, 1},
     "bwd=1 fc=0 fl=0 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=8/8 deep=20/3/3072 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=2731 dump=2731 rb0=2732 xb=5463 ub=5463"},
    {"cartpole B1024 N127", CART, 1024, 127, 0, true, 0, 20, "", {0, 1, 0, 4, 2, 0, 1, 0},
     "bwd=0 fc=1 fl=0 scan=0/1073741824 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=64 dump=64 rb0=0 xb=65 ub=65"},
    {"cartpole B12288 N11 con0", CART, 12288, 11, 0, true, 0, 20, "", {0, 1, 0, 4, 2, 1, 1, 0},
     "bwd=0 fc=1 fl=0 scan=1/1073741824 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=768 dump=768 rb0=0 xb=769 ub=769"},
    {"cartpole B12288 N11 con1", CART, 12288, 11, 2, true, 2, 20, "", {2, 1, 1, 4, 2, 0, 1, 0},
     "bwd=2 fc=0 fl=1 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=768 dump=768 rb0=0 xb=769 ub=769"},
    {"cartpole B20480 N11 con0", CART, 20480, 11, 0, true, 0, 20, "", {2, 1, 1, 4, 2, 0, 1, 2},
     "bwd=2 fc=0 fl=1 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=1280 dump=1280 rb0=0 xb=1281 ub=1281"},
    {"cartpole B20480 N11 con1", CART, 20480, 11, 2, true, 2, 20, "", {2, 1, 1, 4, 2, 0, 1, 2},
     "bwd=2 fc=0 fl=1 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=1280 dump=1280 rb0=0 xb=1281 ub=1281"},
    {"cartpole B32768 N11 con0", CART, 32768, 11, 0, true, 0, 20, "", {2, 1, 1, 4, 2, 0, 1, 2},
     "bwd=2 fc=0 fl=1 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=2/2/1024/2048 waves=2048 dump=2048 rb0=0 xb=2049 ub=2049"},
    {"cartpole B32768 N11 con1", CART, 32768, 11, 2, true, 2, 20, "", {2, 1, 1, 4, 2, 0, 1, 2},
     "bwd=2 fc=0 fl=1 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=2/2/1024/2048 waves=2048 dump=2048 rb0=0 xb=2049 ub=2049"},
    {"cartpole B70000 N11", CART, 70000, 11, 0, true, 0, 20, "", {2, 1, 1, 4, 2, 0, 1, 2},
     "bwd=2 fc=0 fl=1 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=2/2/2188/4376 waves=4376 dump=4376 rb0=0 xb=4377 ub=4377"},
    {"cartpole B64 N11", CART, 64, 11, 0, true, 0, 20, "", {0, 1, 0, 4, 2, 1, 1, 0},
     "bwd=0 fc=1 fl=0 scan=1/1073741824 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=4 dump=4 rb0=0 xb=5 ub=5"},
    {"cartpole B1 N11", CART, 1, 11, 0, true, 0, 20, "", {0, 1, 0, 4, 2, 1, 1, 0},
     "bwd=0 fc=1 fl=0 scan=1/1073741824 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=4 dump=4 rb0=0 xb=5 ub=5"},
    {"quadrotor B40 N11", QUAD, 40, 11, 0, false, 0, 20, "", {1, 0, 1, 16, 2, 0, 1, 1},
     "bwd=1 fc=0 fl=0 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=16/4 deep=20/3/3072 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=22 dump=22 rb0=23 xb=45 ub=45"},
    {"quadrotor B40 N11 con", QUAD, 40, 11, 2, false, 2, 20, "", {1, 0, 1, 16, 2, 0, 1, 1},
     "bwd=1 fc=0 fl=0 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=16/4 deep=20/3/3072 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=22 dump=22 rb0=23 xb=45 ub=45"},
    {"quadrotor B32768 N11", QUAD, 32768, 11, 0, false, 0, 20, "", {1, 0, 1, 2, 2, 0, 1, 1},
     "bwd=1 fc=0 fl=0 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=2/32 deep=20/3/3072 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=10923 dump=10923 rb0=10924 xb=21847 ub=21847"},
    {"quadrotor mrp B40", QATT, 40, 41, 0, false, 0, 20, "", {1, 0, 1, 16, 2, 0, 1, 1},
     "bwd=1 fc=0 fl=0 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=16/4 deep=20/3/3072 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=22 dump=22 rb0=23 xb=45 ub=45"},
    {"quickstart B3", DI2, 3, 21, 4, false, 6, 20, "", {0, 0, 0, 4, 2, 0, 1, 0},
     "bwd=0 fc=1 fl=0 scan=1/1073741824 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=4 dump=4 rb0=0 xb=5 ub=5"},
    {"dint1 B5", DI1, 5, 16, 0, true, 0, 20, "", {0, 1, 0, 4, 2, 1, 1, 0},
     "bwd=0 fc=1 fl=0 scan=1/1073741824 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=4 dump=4 rb0=0 xb=5 ub=5"},
    {"dint2 B5 con", DI2, 5, 16, 2, true, 2, 20, "", {0, 1, 0, 4, 2, 0, 1, 0},
     "bwd=0 fc=1 fl=0 scan=1/1073741824 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=4 dump=4 rb0=0 xb=5 ub=5"},
    {"dint3 B5", DI3, 5, 16, 0, true, 0, 20, "", {0, 0, 0, 4, 2, 0, 1, 0},
     "bwd=0 fc=0 fl=0 scan=0/1073741824 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=4 dump=4 rb0=0 xb=5 ub=5"},
    {"dint2 B32768", DI2, 32768, 16, 0, true, 0, 20, "", {2, 1, 1, 4, 2, 0, 1, 2},
     "bwd=2 fc=0 fl=1 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=2/2/1024/2048 waves=2048 dump=2048 rb0=0 xb=2049 ub=2049"},
    {"hybrid B200", HYB, 200, 11, 0, true, 0, 20, "", {0, 1, 0, 4, 2, 1, 1, 0},
     "bwd=0 fc=1 fl=0 scan=1/1073741824 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=16 dump=16 rb0=0 xb=17 ub=17"},
    {"hybrid B200 con", HYB, 200, 11, 3, true, 2, 20, "", {0, 1, 0, 4, 2, 0, 1, 0},
     "bwd=0 fc=1 fl=0 scan=1/1073741824 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=16 dump=16 rb0=0 xb=17 ub=17"},
    {"hybrid B32768", HYB, 32768, 11, 0, true, 0, 20, "", {2, 1, 1, 4, 2, 0, 1, 2},
     "bwd=2 fc=0 fl=1 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=2/2/1024/2048 waves=2048 dump=2048 rb0=0 xb=2049 ub=2049"},
    {"vector B70", VEC, 70, 14, 0, true, 0, 20, "", {0, 0, 0, 4, 2, 0, 1, 0},
     "bwd=0 fc=0 fl=0 scan=0/1073741824 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=8 dump=8 rb0=0 xb=9 ub=9"},
    {"vector B70 con", VEC, 70, 14, 2, true, 2, 20, "", {0, 0, 0, 4, 2, 0, 1, 0},
     "bwd=0 fc=0 fl=0 scan=0/1073741824 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=8 dump=8 rb0=0 xb=9 ub=9"},
    {"vector B32768", VEC, 32768, 14, 0, true, 0, 20, "", {0, 0, 0, 4, 2, 0, 1, 0},
     "bwd=0 fc=0 fl=0 scan=0/1073741824 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=2/2/1024/2048 waves=2048 dump=2048 rb0=0 xb=2049 ub=2049"},
    {"cartpole B1024 LS_CANDIDATES=2", CART, 1024, 11, 0, true, 0, 20, "LS_CANDIDATES=2", {0, 1, 0, 2, 2, 1, 1, 0},
     "bwd=0 fc=1 fl=0 scan=1/1073741824 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=2/32 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=32 dump=32 rb0=0 xb=33 ub=33"},
    {"cartpole B1024 LS_CANDIDATES=3", CART, 1024, 11, 0, true, 0, 20, "LS_CANDIDATES=3", {0, 1, 0, 3, 2, 1, 1, 0},
     "bwd=0 fc=1 fl=0 scan=1/1073741824 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=3/21 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=49 dump=49 rb0=0 xb=50 ub=50"},
    {"quadrotor B4096 LS_CANDIDATES=8", QUAD, 4096, 11, 0, false, 0, 20, "LS_CANDIDATES=8", {1, 0, 1, 8, 2, 0, 1, 1},
     "bwd=1 fc=0 fl=0 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=8/8 deep=20/3/3072 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=1366 dump=1366 rb0=1367 xb=2733 ub=2733"},
    {"quadrotor B4096 LS_CANDIDATES=3", QUAD, 4096, 11, 0, false, 0, 20, "LS_CANDIDATES=3", {1, 0, 1, 2, 2, 0, 1, 1},
     "bwd=1 fc=0 fl=0 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=2/32 deep=20/3/3072 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=1366 dump=1366 rb0=1367 xb=2733 ub=2733"},
    {"quadrotor B4096 LS_DEEP=0", QUAD, 4096, 11, 0, false, 0, 20, "LS_DEEP=0", {1, 0, 1, 16, 2, 0, 1, 1},
     "bwd=1 fc=0 fl=0 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=16/4 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=1024 dump=1024 rb0=1025 xb=2049 ub=2049"},
    {"cartpole B1024 SCAN=0", CART, 1024, 11, 0, true, 0, 20, "SCAN=0", {0, 1, 0, 4, 2, 0, 1, 0},
     "bwd=0 fc=1 fl=0 scan=0/1073741824 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=64 dump=64 rb0=0 xb=65 ub=65"},
    {"cartpole B1024 SCAN=2", CART, 1024, 11, 0, true, 0, 20, "SCAN=2", {0, 1, 0, 4, 2, 1, 1, 0},
     "bwd=0 fc=1 fl=0 scan=2/1073741824 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=64 dump=64 rb0=0 xb=65 ub=65"},
    {"cartpole B20480 SCAN=0", CART, 20480, 11, 0, true, 0, 20, "SCAN=0", {2, 1, 1, 4, 2, 0, 1, 2},
     "bwd=2 fc=0 fl=1 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=1280 dump=1280 rb0=0 xb=1281 ub=1281"},
    {"cartpole B12288 SCAN=0", CART, 12288, 11, 0, true, 0, 20, "SCAN=0", {2, 1, 1, 4, 2, 0, 1, 0},
     "bwd=2 fc=0 fl=1 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=768 dump=768 rb0=0 xb=769 ub=769"},
    {"cartpole B1024 BACKWARD=lane", CART, 1024, 11, 0, true, 0, 20, "BACKWARD=lane", {2, 1, 1, 4, 2, 0, 1, 0},
     "bwd=2 fc=0 fl=1 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=64 dump=64 rb0=0 xb=65 ub=65"},
    {"cartpole B1024 BACKWARD=mfma", CART, 1024, 11, 0, true, 0, 20, "BACKWARD=mfma", {1, 0, 1, 4, 2, 0, 1, 0},
     "bwd=1 fc=0 fl=0 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=64 dump=64 rb0=0 xb=65 ub=65"},
    {"cartpole B32768 BACKWARD=coop", CART, 32768, 11, 0, true, 0, 20, "BACKWARD=coop", {0, 1, 0, 4, 2, 1, 1, 0},
     "bwd=0 fc=1 fl=0 scan=1/1073741824 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=2/2/1024/2048 waves=2048 dump=2048 rb0=0 xb=2049 ub=2049"},
    {"quadrotor B4096 BACKWARD=coop", QUAD, 4096, 11, 0, false, 0, 20, "BACKWARD=coop", {1, 0, 1, 16, 2, 0, 1, 1},
     "bwd=1 fc=0 fl=0 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=16/4 deep=20/3/3072 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=1366 dump=1366 rb0=1367 xb=2733 ub=2733"},
    {"cartpole B32768 EXPAND_LANE=0", CART, 32768, 11, 0, true, 0, 20, "EXPAND_LANE=0", {2, 1, 1, 4, 2, 0, 1, 2},
     "bwd=2 fc=0 fl=1 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=0 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=2/2/1024/2048 waves=2048 dump=2048 rb0=0 xb=2049 ub=2049"},
    {"cartpole B1024 FUSED_COOP=0", CART, 1024, 11, 0, true, 0, 20, "FUSED_COOP=0", {0, 0, 0, 4, 2, 0, 1, 0},
     "bwd=0 fc=0 fl=0 scan=0/1073741824 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=64 dump=64 rb0=0 xb=65 ub=65"},
    {"cartpole B1024 ACCEPT_ROLL_MIN=0", CART, 1024, 11, 0, true, 0, 20, "ACCEPT_ROLL_MIN=0", {0, 1, 0, 4, 2, 1, 0, 0},
     "bwd=0 fc=1 fl=0 scan=1/1073741824 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=0/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=64 dump=64 rb0=0 xb=65 ub=65"},
    {"quadrotor B4096 ACCEPT_ROLL_MIN=1", QUAD, 4096, 11, 0, false, 0, 20, "ACCEPT_ROLL_MIN=1", {1, 0, 1, 16, 2, 0, 1, 1},
     "bwd=1 fc=0 fl=0 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=16/4 deep=20/3/3072 roll=1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=1366 dump=1366 rb0=1367 xb=2733 ub=2733"},
    {"cartpole B32768 ACCEPT_ROLL_FRAC=0", CART, 32768, 11, 0, true, 0, 20, "ACCEPT_ROLL_FRAC=0", {2, 1, 1, 4, 2, 0, 1, 2},
     "bwd=2 fc=0 fl=1 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0 rp=16384/0.7 ls2=2/2/1024/2048 waves=2048 dump=2048 rb0=0 xb=2049 ub=2049"},
    {"cartpole B32768 REPACK=0", CART, 32768, 11, 0, true, 0, 20, "REPACK=0", {2, 1, 1, 4, 2, 0, 1, 0},
     "bwd=2 fc=0 fl=1 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=0/0.7 ls2=2/2/1024/2048 waves=2048 dump=2048 rb0=0 xb=2049 ub=2049"},
    {"cartpole B12288 REPACK=2048 BACKWARD=lane", CART, 12288, 11, 0, true, 0, 20, "REPACK=2048 BACKWARD=lane", {2, 1, 1, 4, 2, 0, 1, 2},
     "bwd=2 fc=0 fl=1 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=2048/0.7 ls2=0/2/0/0 waves=768 dump=768 rb0=0 xb=769 ub=769"},
    {"cartpole B32768 REPACK_AT=0.3", CART, 32768, 11, 0, true, 0, 20, "REPACK_AT=0.3", {2, 1, 1, 4, 2, 0, 1, 2},
     "bwd=2 fc=0 fl=1 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.3 ls2=2/2/1024/2048 waves=2048 dump=2048 rb0=0 xb=2049 ub=2049"},
    {"quadrotor B4096 EXPAND_PACK=0", QUAD, 4096, 11, 0, false, 0, 20, "EXPAND_PACK=0", {1, 0, 1, 16, 2, 0, 1, 1},
     "bwd=1 fc=0 fl=0 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=0 elane=1 cw=16/4 deep=20/3/3072 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=1366 dump=1366 rb0=1367 xb=2733 ub=2733"},
    {"cartpole B1024 FWD2=0", CART, 1024, 11, 0, true, 0, 20, "FWD2=0", {0, 1, 0, 4, 1, 1, 1, 0},
     "bwd=0 fc=1 fl=0 scan=1/1073741824 cmp=0 fwd2=0 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=64 dump=64 rb0=0 xb=65 ub=65"},
    {"quadrotor B4096 FWD2=1", QUAD, 4096, 11, 0, false, 0, 20, "FWD2=1", {1, 0, 1, 16, 2, 0, 1, 1},
     "bwd=1 fc=0 fl=0 scan=0/1073741824 cmp=1 fwd2=1 mrg=1 pack=1 elane=1 cw=16/4 deep=20/3/3072 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=1366 dump=1366 rb0=1367 xb=2733 ub=2733"},
    {"quadrotor B4096 FWD2=7", QUAD, 4096, 11, 0, false, 0, 20, "FWD2=7", {1, 0, 1, 16, 2, 0, 1, 1},
     "bwd=1 fc=0 fl=0 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=16/4 deep=20/3/3072 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=1366 dump=1366 rb0=1367 xb=2733 ub=2733"},
    {"cartpole B1024 COOP_MERGE=0", CART, 1024, 11, 0, true, 0, 20, "COOP_MERGE=0", {0, 1, 0, 4, 2, 1, 1, 0},
     "bwd=0 fc=1 fl=0 scan=1/1073741824 cmp=0 fwd2=2 mrg=0 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=64 dump=64 rb0=0 xb=65 ub=65"},
    {"cartpole B1024 SCAN_MAX=100", CART, 1024, 11, 0, true, 0, 20, "SCAN_MAX=100", {0, 1, 0, 4, 2, 1, 1, 0},
     "bwd=0 fc=1 fl=0 scan=1/100 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=64 dump=64 rb0=0 xb=65 ub=65"},
    {"cartpole B32768 FUSED_LANE=0", CART, 32768, 11, 0, true, 0, 20, "FUSED_LANE=0", {2, 0, 0, 4, 2, 0, 1, 0},
     "bwd=2 fc=0 fl=0 scan=0/1073741824 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=2/2/1024/2048 waves=2048 dump=2048 rb0=0 xb=2049 ub=2049"},
    {"quadrotor B4096 LS_REPACK=0", QUAD, 4096, 11, 0, false, 0, 20, "LS_REPACK=0", {1, 0, 1, 16, 2, 0, 1, 0},
     "bwd=1 fc=0 fl=0 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=16/4 deep=20/3/3072 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=1366 dump=1366 rb0=0 xb=1367 ub=1367"},
    {"cartpole B32768 LS_TWO=0", CART, 32768, 11, 0, true, 0, 20, "LS_TWO=0", {2, 1, 1, 4, 2, 0, 1, 2},
     "bwd=2 fc=0 fl=1 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=2048 dump=2048 rb0=0 xb=2049 ub=2049"},
    {"cartpole B32768 LS_TWO=1,4", CART, 32768, 11, 0, true, 0, 20, "LS_TWO=1,4", {2, 1, 1, 4, 2, 0, 1, 2},
     "bwd=2 fc=0 fl=1 scan=0/1073741824 cmp=1 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=1/4/512/2560 waves=2048 dump=2048 rb0=0 xb=2049 ub=2561"},
    {"quadrotor B4096 COMPACT=0", QUAD, 4096, 11, 0, false, 0, 20, "COMPACT=0", {1, 0, 0, 16, 2, 0, 1, 1},
     "bwd=1 fc=0 fl=0 scan=0/1073741824 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=16/4 deep=20/3/3072 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=1366 dump=1366 rb0=1367 xb=2733 ub=2733"},
    {"cartpole B32768 COMPACT=0", CART, 32768, 11, 0, true, 0, 20, "COMPACT=0", {2, 1, 0, 4, 2, 0, 1, 0},
     "bwd=2 fc=0 fl=1 scan=0/1073741824 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=2/2/1024/2048 waves=2048 dump=2048 rb0=0 xb=2049 ub=2049"},
    {"cartpole B1024 FULL_COST_BLOCKS=1", CART, 1024, 11, 0, true, 0, 20, "FULL_COST_BLOCKS=1", {0, 0, 0, 4, 2, 0, 1, 0},
     "bwd=0 fc=1 fl=0 scan=1/1073741824 cmp=0 fwd2=2 mrg=1 pack=1 elane=1 cw=4/16 deep=0/0/0 roll=-1/0.25 rp=16384/0.7 ls2=0/2/0/0 waves=64 dump=64 rb0=0 xb=65 ub=65"},
};

static void pinned_rows() {
  for (const Row& r : ROWS) {
    const Model& M = MODELS[r.model];
    const PathKnobs k = knobs(r.env);
    const PathPlan p = plan_paths(M.t, shape(M, r.B, r.N, r.n_cons, r.diag, r.ls), k);
    const bool full = g_env.count("TRAJOPT_FULL_COST_BLOCKS") && g_env["TRAJOPT_FULL_COST_BLOCKS"] != "0";
    int32_t info[8];
    path_report(p, M.t, h_diag_of(p, r.diag, full), r.ev, r.B, info);
    for (int i = 0; i < 8; ++i) CHECK(info[i] == r.info[i], "row '%s': info[%d] = %d, pinned %d", r.name, i, info[i], r.info[i]);
    if (r.plan) CHECK(plan_text(p) == r.plan, "row '%s': plan\n  is     %s\n  pinned %s", r.name, plan_text(p).c_str(), r.plan);
  }
  printf("rows %d\n", (int)(sizeof(ROWS) / sizeof(ROWS[0])));
}

// ---- (b) invariants ------------------------------------------------------------------------------------------------------------------
static long long n_plans = 0, n_steps = 0, kind_count[4] = {0, 0, 0, 0}, deep_steps[2] = {0, 0}, two_wave_steps[2] = {0, 0}, store_steps[2] = {0, 0},
                 two_launch_steps[2] = {0, 0}, scan_side[2] = {0, 0};

static bool same_step(const StepPlan& a, const StepPlan& b) { return a.kind == b.kind && a.CW == b.CW && a.TW == b.TW && a.two_wave == b.two_wave && a.store_x == b.store_x && a.two_launch == b.two_launch; }
static void check_step(const PathPlan& p, const Model& M, const StepPlan& s, int Bp_now, const char* what) {
  ++kind_count[s.kind]; ++deep_steps[s.CW == p.cw_deep]; ++two_wave_steps[s.two_wave]; ++store_steps[s.store_x]; ++two_launch_steps[s.two_launch];
  CHECK(s.CW >= 1 && s.TW >= 1 && s.CW * s.TW <= 64, "%s: step shape %d x %d", what, s.CW, s.TW);
  // the forward launch of this step: ceil(Bp / TW) blocks, dump block behind them, repacked round behind that (own arithmetic)
  const long long blocks = ((long long)Bp_now + s.TW - 1) / s.TW;
  CHECK(blocks <= p.waves && blocks <= p.dump_wave, "%s: %lld forward blocks, %lld allocated, dump block %d", what, blocks, p.waves, p.dump_wave);
  CHECK(p.dump_wave < p.x_blocks && p.dump_wave < p.u_blocks, "%s: dump block outside the candidates", what);
  if (p.repack_block0) CHECK(p.repack_block0 > p.dump_wave && p.repack_block0 + blocks <= p.x_blocks && p.repack_block0 + blocks <= p.u_blocks, "%s: repacked round outside the candidates", what);
  if (s.two_launch) {
    CHECK(!s.store_x && p.ls2_cwa >= 1 && p.ls2_cwb >= 1 && p.ls2_cwa * (64 / p.ls2_cwa) <= 64 && p.ls2_cwb * (64 / p.ls2_cwb) <= 64, "%s: two-launch widths", what);
    const long long nA = ((long long)Bp_now + 64 / p.ls2_cwa - 1) / (64 / p.ls2_cwa), nB = ((long long)Bp_now + 64 / p.ls2_cwb - 1) / (64 / p.ls2_cwb);
    CHECK(nA <= p.ls2_blkA && p.ls2_blkA + nB <= p.ls2_dump && p.ls2_dump < p.u_blocks, "%s: two-launch blocks %lld + %lld, A %d dump %d of %lld", what, nA, nB, p.ls2_blkA, p.ls2_dump, p.u_blocks);
  }
  if (s.kind == STEP_FUSED_LANE) CHECK(M.t.expand_backward && p.bwd_lane, "%s: fused lane step without its kernel", what);
  if (s.kind == STEP_FUSED_COOP) CHECK(M.t.expand_backward_coop && !p.bwd_lane && !p.bwd_mfma, "%s: fused cooperative step without its kernel", what);
  if (s.kind == STEP_SCAN) CHECK(M.t.expand_backward_scan && !p.bwd_lane && !p.bwd_mfma, "%s: scan step without its kernel", what);
  if (!s.store_x) CHECK(M.t.accept_roll && !s.two_wave, "%s: controls-only step without k_accept_roll / in a two-wave workgroup", what);
}

static void check_plan(const Model& M, const PathShape& sh, const PathKnobs& k, bool diag, const char* env, bool every_count) {
  ++n_plans;
  const PathPlan p = plan_paths(M.t, sh, k);
  char what[256];
  snprintf(what, sizeof what, "%s B=%d cons=%d diag=%d [%s]", M.name, sh.B, sh.n_cons, (int)diag, env);
  CHECK(!(p.bwd_mfma && p.bwd_lane), "%s: mfma and lane", what);
  CHECK(!p.bwd_mfma || M.t.mfma_backward, "%s: mfma not compiled", what);
  CHECK(!p.bwd_lane || M.t.lane_backward, "%s: lane not compiled", what);
  CHECK(p.bwd_mfma || p.bwd_lane || M.t.coop_backward, "%s: cooperative not compiled", what);
  CHECK(!p.fused_lane || p.bwd_lane, "%s: fused_lane without lane", what);
  CHECK(!p.fused_coop || (!p.bwd_lane && !p.bwd_mfma), "%s: fused_coop on another flavour", what);
  CHECK(!p.scan || p.fused_coop, "%s: scan without fused_coop", what);
  CHECK(p.cw_base * p.tw_base <= 64 && p.cw_base >= 1 && p.tw_base >= 1, "%s: base shape", what);
  CHECK(p.cw_deep == 0 || (p.cw_deep * p.tw_deep <= 64 && p.tw_deep >= 2), "%s: deep shape", what);
  CHECK(p.fwd2 >= 0 && p.fwd2 <= 2, "%s: fwd2", what);
  CHECK(p.u_blocks >= p.x_blocks, "%s: fewer control blocks than state blocks", what);
  const int ev = sh.n_cons ? 2 : 0, hd = h_diag_of(p, diag);
  // every active count of the full batch, and of the working sets a repacking solve moves into (B = count, Bp = count rounded up)
  std::vector<int> sets = {sh.B};
  if (working_set_repack(p, M.t)) for (int b = sh.B / 2; b >= 1; b /= 3) sets.push_back(b);
  for (int Bnow : sets) {
    const int Bp_now = (Bnow + 63) / 64 * 64;
    // every active count 0 .. B of the full batch (plans with at most one knob set, diagonal cost blocks, default search depth); the other
    // plans and the working sets: a stride plus both sides of every threshold the step plan compares the count with
    const int stride = (every_count && Bnow == sh.B) || Bnow <= 256 ? 1 : Bnow / 251 + 1;
    const int thr[] = {Bnow, p.deep_max_active, p.scan_max_active, roll_min(p, M.t), (int)(p.roll_min_frac * Bnow), p.simds * p.tw_base / 2, p.simds * (p.tw_deep ? p.tw_deep : 1) / 2};
    for (int compact_armed = p.ls2_cwa ? 0 : p.compact; compact_armed <= p.compact; ++compact_armed) {  // (armed or not matters to the two-launch search only)
      StepPlan prev = StepPlan();
      bool first = true;
      auto visit = [&](int la) {  // (the checks see the step plan only: a run of equal plans is checked once)
        const StepPlan s = plan_step(p, M.t, hd, ev, compact_armed, la, Bnow);
        ++n_steps;
        if (!first && same_step(s, prev)) return;
        check_step(p, M, s, Bp_now, what);
        prev = s; first = false;
      };
      for (int la = 0; la <= Bnow; la += stride) visit(la);
      if (stride > 1) for (int t : thr) for (int d = -2; d <= 2; ++d) if (t + d >= 0 && t + d <= Bnow) visit(t + d);
    }
  }
  // the report agrees with the step plan on fused / scan / accept-roll, on either side of each threshold
  int32_t info[8];
  path_report(p, M.t, hd, ev, sh.B, info);
  const int la_list[] = {0, 1, p.scan_max_active - 1, p.scan_max_active, p.scan_max_active + 1, roll_min(p, M.t) - 1, roll_min(p, M.t), sh.B / 2, sh.B - 1, sh.B};
  for (int la : la_list) {
    if (la < 0 || la > sh.B) continue;
    const StepPlan s = plan_step(p, M.t, hd, ev, p.compact, la, sh.B);
    CHECK((s.kind != STEP_SPLIT) == (info[1] == 1), "%s: report says fused=%d, step at %d active is kind %d", what, info[1], la, (int)s.kind);
    if (s.kind == STEP_SCAN) { CHECK(info[5] == 1, "%s: scan step, report says none", what); ++scan_side[0]; }
    else if (info[5] == 1) { CHECK(la > p.scan_max_active, "%s: report says scan, step at %d active (max %d) is kind %d", what, la, p.scan_max_active, (int)s.kind); ++scan_side[1]; }
    if (!s.store_x) CHECK(info[6] == 1, "%s: controls-only step, report says none", what);
  }
  CHECK(info[0] == (p.bwd_mfma ? 1 : p.bwd_lane ? 2 : 0) && info[2] == p.compact && info[3] == p.cw_base, "%s: report flavour / compact / width", what);
}

static void sweep() {
  // every knob unset (the first entry) or at each of its extreme values
  const std::vector<std::vector<const char*>> knob_values = {
      {"", "LS_CANDIDATES=-5", "LS_CANDIDATES=1", "LS_CANDIDATES=3", "LS_CANDIDATES=16", "LS_CANDIDATES=99"}, {"", "LS_DEEP=0", "LS_DEEP=1"},
      {"", "SCAN=0", "SCAN=1", "SCAN=2"}, {"", "BACKWARD=coop", "BACKWARD=mfma", "BACKWARD=lane", "BACKWARD=other"}, {"", "EXPAND_LANE=0", "EXPAND_LANE=1"},
      {"", "FUSED_COOP=0", "FUSED_COOP=1"}, {"", "ACCEPT_ROLL_MIN=0", "ACCEPT_ROLL_MIN=1", "ACCEPT_ROLL_MIN=2000000000", "ACCEPT_ROLL_MIN=-3"},
      {"", "ACCEPT_ROLL_FRAC=0", "ACCEPT_ROLL_FRAC=1", "ACCEPT_ROLL_FRAC=7"}, {"", "REPACK=0", "REPACK=1", "REPACK=2000000000"}, {"", "REPACK_AT=0", "REPACK_AT=1"},
      {"", "EXPAND_PACK=0", "EXPAND_PACK=1"}, {"", "FWD2=0", "FWD2=1", "FWD2=2", "FWD2=-1", "FWD2=9"}, {"", "COOP_MERGE=0", "COOP_MERGE=1"},
      {"", "SCAN_MAX=0", "SCAN_MAX=100", "SCAN_MAX=2000000000"}, {"", "FUSED_LANE=0", "FUSED_LANE=1"}, {"", "LS_REPACK=0", "LS_REPACK=1"},
      {"", "LS_TWO=0", "LS_TWO=1", "LS_TWO=1,1", "LS_TWO=16,16", "LS_TWO=17,2", "LS_TWO=2,17", "LS_TWO=3,5", "LS_TWO=64"}, {"", "COMPACT=0", "COMPACT=1"}};
  const int Bs[] = {1, 63, 64, 65, 1024, 12288, 20480, 32768, 70000};
  for (const Model& M : MODELS)
    for (int B : Bs)
      for (int cons = 0; cons <= 2; cons += 2)
        for (int diag = 0; diag <= 1; ++diag)
          for (int ls : {20, 1, 40})
            for (const auto& kv : knob_values)
              for (size_t i = ls == 20 ? 0 : 1; i < kv.size(); ++i) {  // (the all-unset plan once per line-search depth is enough)
                if (i == 0 && &kv != &knob_values[0]) continue;
                // the second knob of a pair: the ones that interact with most others
                for (const char* with : {"", "BACKWARD=lane", "ACCEPT_ROLL_MIN=1 ACCEPT_ROLL_FRAC=0", "FWD2=0 REPACK=64"}) {
                  const std::string env = std::string(kv[i]) + (*kv[i] && *with ? " " : "") + with;
                  if (*with && std::string(kv[i]).substr(0, std::string(kv[i]).find('=')) == std::string(with).substr(0, std::string(with).find('='))) continue;
                  const PathKnobs k = knobs(env.c_str());
                  check_plan(M, shape(M, B, 41, cons, diag != 0, ls), k, diag != 0, env.c_str(), !*with && ls == 20 && diag);
                }
              }
  // other devices: the thresholds scale with the compute units
  for (int cus : {1, 64, 304})
    for (const Model& M : MODELS)
      for (int B : Bs) check_plan(M, shape(M, B, 41, 0, true, 20, cus), knobs(""), true, "cus", true);
}

static void forward_modes() {
  // every mask over the variants a model can compile x every request: never a variant whose bit is clear, -1 exactly when the chain
  // (as asked; without the pinned-RK4 bit; with the unit-SOC bit; the general variant) holds nothing
  const uint32_t masks[] = {F_SMALL, F_QUAD, F_ATT, 0u, 1u, 1u << 8, 1u << 10, 0xFFFFFFFFu, 0x00FF00FFu, 1u << 12, (1u << 9) | (1u << 17)};
  long long found = 0, none = 0;
  for (uint32_t mask : masks)
    for (int req = 0; req < 32; ++req) {
      const bool simple = req & 1, cons = req & 2, rk4 = req & 4, general = req & 8, unit = req & 16;
      const int mode = forward_mode(simple, cons, rk4, general, unit, mask);
      int m0 = (req & 15);
      auto has = [&](int m) { return (mask >> m) & 1u; };
      if (!has(m0)) m0 &= ~4;
      const int cand[] = {unit && has(m0 | 16) ? (m0 | 16) : m0, (m0 | 8) & ~1 & ~16};  // own restatement of the chain's two ends
      const bool any = has(cand[0]) || has(cand[1]);
      CHECK((mode >= 0) == any, "forward_mode(req %d, mask %08x) = %d, a fallback %s", req, mask, mode, any ? "exists" : "does not exist");
      if (mode >= 0) {
        ++found;
        CHECK(has(mode), "forward_mode(req %d, mask %08x) = %d: not compiled", req, mask, mode);
        CHECK(mode == (has(cand[0]) ? cand[0] : cand[1]), "forward_mode(req %d, mask %08x) = %d", req, mask, mode);
        CHECK(((mode & 2) != 0) == cons, "forward_mode(req %d, mask %08x) = %d: constraint bit changed", req, mask, mode);
      } else ++none;
    }
  // the request launch_forward makes with one plant per trajectory (general variant, stage cost read per knot) over every model's mask of
  // flagged variants: a compiled general variant with the constraint bit as asked, -1 exactly for the models without flagged instances
  for (const Model& M : MODELS)
    for (int req = 0; req < 4; ++req) {
      const bool cons = req & 1, rk4 = req & 2;
      const uint32_t mask = M.t.forward_plants;
      const int mode = forward_mode(false, cons, rk4, true, false, mask);
      CHECK((mode >= 0) == (mask != 0), "%s: plants forward_mode(cons %d, rk4 %d, mask %08x) = %d", M.name, (int)cons, (int)rk4, mask, mode);
      if (mode >= 0) {
        ++found;
        CHECK(((mask >> mode) & 1u) && (mode & 8) && !(mode & 1) && ((mode & 2) != 0) == cons, "%s: plants forward_mode(cons %d, rk4 %d, mask %08x) = %d", M.name, (int)cons, (int)rk4, mask, mode);
      } else ++none;
    }
  printf("forward_found %lld forward_none %lld\n", found, none);
}

static void compaction() {
  long long one = 0, two = 0, refused = 0;
  auto check = [&](long long Bp) {
    int per = 0, nb = 0;
    const bool ok = compact_grid((int)Bp, &per, &nb);
    if (Bp <= COMPACT_ONE_LAUNCH) ++one;
    if (Bp > 16777216) { CHECK(!ok, "compact_grid(%lld) accepted", Bp); ++refused; return; }
    ++two;
    CHECK(ok && nb >= 1 && nb <= 256 && per % 1024 == 0 && per >= 1024 && per <= 65536, "compact_grid(%lld): per %d nb %d", Bp, per, nb);
    CHECK((long long)per * nb >= Bp && (long long)per * (nb - 1) < Bp, "compact_grid(%lld): %d x %d does not cover / leaves an idle workgroup", Bp, per, nb);
  };
  for (long long Bp = 64; Bp <= 16777216 + 64 * 64; Bp += 64) check(Bp);
  for (long long Bp : {33554432ll, 1073741824ll}) check(Bp);
  printf("compact_one %lld compact_two %lld compact_refused %lld\n", one, two, refused);
}

int main() {
  pinned_rows();
  sweep();
  forward_modes();
  compaction();
  printf("plans %lld steps %lld\n", n_plans, n_steps);
  printf("split %lld fused_lane %lld fused_coop %lld scan %lld\n", kind_count[STEP_SPLIT], kind_count[STEP_FUSED_LANE], kind_count[STEP_FUSED_COOP], kind_count[STEP_SCAN]);
  printf("base_shape %lld deep_shape %lld one_wave %lld two_wave %lld store_x %lld controls_only %lld one_launch %lld two_launch %lld\n", deep_steps[0], deep_steps[1],
         two_wave_steps[0], two_wave_steps[1], store_steps[1], store_steps[0], two_launch_steps[0], two_launch_steps[1]);
  printf("scan_below_max %lld scan_above_max %lld\n", scan_side[0], scan_side[1]);
  printf("checks %lld fails %lld\n", checks, fails);
  return fails ? 1 : 0;
}
