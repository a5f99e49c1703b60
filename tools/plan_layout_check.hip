// plan_layout_check.hip -- a stand-alone host program around m2t_plan_layout.h (the region table of an m2t_plan and its three
// readers), for a sanitizer run of that HOST code on a machine without a device.  The table holds pointers into the handle structs
// and the placements write through them, so a slot past the end of a handle array is what such a run is for:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/plan_layout_check.hip -o plan_layout_check
//   ./plan_layout_check
//
// It links nothing of the library: the header is host-only.  Plans: (2, 40, 56) padded to 64 x 64, dtype {fp32, bf16} x scale
// {2, 3, 4} x depth {1, 2, 3, 8}; modes: training, inference, inference with local_norm 8 and 64, health 1 and 2; under every mode
// each combination of the schedule fields a region predicate reads.  After every resolve: each region starts on a 256-byte
// boundary, the placed regions do not overlap and tile [0, workspace_bytes), every name that shares a placed region's offset (an
// alias of the inference layout) has that region's count, every handle has a declaration, a placed declaration's handle is its
// offset and every other handle is M2T_NO_REGION, and a health row's offset and count are its region's.  The transitions of
// tests/test_plan_layout_cpu.py are walked on ONE handle set and must end in what a fresh one resolves to.  Exit status 0 = every
// expectation held.
#include <cstdio>
#include "../m2trans_amd/csrc/m2t_plan_layout.h"

static int failures = 0;
#define EXPECT(cond)                                                                    \
  do {                                                                                  \
    if (!(cond)) {                                                                      \
      if (++failures <= 20) fprintf(stderr, "line %d: expectation failed: %s\n", __LINE__, #cond); \
    }                                                                                   \
  } while (0)

struct Plan {
  m2t_plan_geom g;
  m2t_sched s;
  m2t_plan_handles hd;
  m2t_region ws;
  m2t_health_table ht;
  void resolve() { m2t_resolve_workspace(g, s, hd, ws, ht); }
};

static Plan make_plan(int dt, int scale, int nb) {
  Plan p{};
  m2t_plan_geom& g = p.g;
  g.B = 2; g.H0 = 40; g.W0 = 56; g.H = 64; g.W = 64; g.scale = scale; g.nb = nb; g.dt = dt;
  g.esz = dt == M2T_F32 ? 4 : 2;
  g.P = (long long)g.H * g.W;
  g.Hs = g.H0 * scale; g.Ws = g.W0 * scale; g.Hsp = g.H * scale; g.Wsp = g.W * scale;
  // the sizes m2t_plan_create takes from the pack registration and the kernels: any numbers do for the invariants
  g.n_pack_descs = 18 * nb + (scale == 4 ? 4 : 2);
  g.n_pack_block_ints = 2 * 37 * g.n_pack_descs;
  g.npacked = 1234567 * (size_t)nb + 4099;
  g.nparams = 617283 * (size_t)nb + 7001;
  g.vring_elems = (size_t)g.B * (g.H / 32) * (g.W / 32) * 36 * 256;
  g.arena_floats = 1000003 * (size_t)nb + 12345;
  p.hd.blk.assign(nb, m2t_block_handles{});
  return p;
}

static void check(Plan& p) {
  const m2t_plan_geom& g = p.g;
  m2t_plan_handles ref;                          // the declarations again, on a handle set of their own: sizes by name
  ref.blk.assign(g.nb, m2t_block_handles{});
  m2t_clear_workspace_handles(ref);
  const m2t_plan_table tb = m2t_plan_regions(g, p.s, ref);
  const m2t_plan_table mine = m2t_plan_regions(g, p.s, p.hd);      // ... and on the plan's: the slots
  std::map<std::string, const m2t_region_decl*> by_name;
  for (const m2t_region_decl& d : tb.regions) by_name[d.name] = &d;
  EXPECT(by_name.size() == tb.regions.size());
  // every handle has a declaration (t2act, t2der and g_t2pre exist at x4 only)
  size_t slots = 0;
  for (const m2t_region_decl& d : tb.regions) slots += d.slot != nullptr;
  const size_t handles = (sizeof(m2t_plan_ws) - sizeof(std::vector<size_t>)) / sizeof(size_t) + (g.nb + 1) +
                         (size_t)g.nb * (sizeof(m2t_block_ws) / sizeof(size_t));
  EXPECT(slots == handles - (g.scale == 4 ? 0 : 3));
  EXPECT(p.hd.X.size() == (size_t)g.nb + 1 && p.hd.blk.size() == (size_t)g.nb);
  // placed regions by offset; a second name at an offset is an alias and must agree with the first
  std::map<size_t, size_t> placed;               // offset -> bytes
  for (const auto& kv : p.ws.t) {
    auto it = by_name.find(kv.first);
    EXPECT(it != by_name.end());
    if (it == by_name.end()) continue;
    const size_t nbytes = kv.second.n * it->second->es;
    EXPECT(kv.second.off % 256 == 0 && kv.second.n == it->second->n);
    auto ins = placed.insert({kv.second.off, nbytes});
    EXPECT(ins.second || (g.inference && ins.first->second == nbytes));
  }
  size_t end = 0;
  for (const auto& kv : placed) {
    EXPECT(kv.first == ((end + 255) & ~(size_t)255));
    end = kv.first + kv.second;
  }
  EXPECT(p.ws.bytes == ((end + 255) & ~(size_t)255));
  // handles: the offset of a placed name, absent otherwise
  for (const m2t_region_decl& d : mine.regions) {
    auto it = p.ws.t.find(d.name);
    if (d.slot) EXPECT(*d.slot == (it == p.ws.t.end() ? M2T_NO_REGION : it->second.off));
    const bool training_class = d.cls <= M2T_RC_BACKWARD;
    if (!g.inference) EXPECT((it != p.ws.t.end()) == (training_class || (d.cls == M2T_RC_HEALTH && g.health > 0)));
    else EXPECT((it != p.ws.t.end()) == d.fwd_reads);
  }
  // health rows
  EXPECT(p.ht.descs.size() == p.ht.names.size() && (g.health > 0 && !g.inference) == !p.ht.descs.empty());
  int items = 0;
  for (size_t r = 0; r < p.ht.descs.size(); ++r) {
    const m2t_health_desc& d = p.ht.descs[r];
    EXPECT(d.item0 == items && d.nitems >= 1 && d.phase == ((int)r >= p.ht.rows_fwd));
    items += d.nitems;
    if (d.off < 0) { EXPECT(p.ht.names[r] == "sr" || p.ht.names[r] == "grads"); continue; }
    auto it = p.ws.t.find(p.ht.names[r]);
    EXPECT(it != p.ws.t.end() && (size_t)d.off == it->second.off && (size_t)d.n == it->second.n);
  }
  EXPECT((size_t)items * 2 == p.ht.work.size());
}

static bool same(const Plan& a, const Plan& b) {
  if (a.ws.bytes != b.ws.bytes || a.ws.t.size() != b.ws.t.size() || a.ht.names != b.ht.names || a.ht.work != b.ht.work) return false;
  for (const auto& kv : a.ws.t) {
    auto it = b.ws.t.find(kv.first);
    if (it == b.ws.t.end() || it->second.off != kv.second.off || it->second.n != kv.second.n) return false;
  }
  for (size_t r = 0; r < a.ht.descs.size(); ++r)
    if (a.ht.descs[r].off != b.ht.descs[r].off || a.ht.descs[r].n != b.ht.descs[r].n) return false;
  return a.hd.X == b.hd.X && a.hd.arena == b.hd.arena && a.hd.health == b.hd.health && a.hd.xn == b.hd.xn;
}

// schedule number c of the combinations of the fields the region predicates read
static const int N_SCHED = 2 * 3 * 2 * 2 * 2 * 3 * 3;
static m2t_sched sched(int c, int scale) {
  m2t_sched s{};
  s.c16_fused_fwd = c % 2; c /= 2;
  const int c64 = c % 3; c /= 3;                 // unfused, fused, fused with branch_prep inside
  s.c64_fused_fwd = c64 >= 1; s.prep_in_fwd = c64 == 2;
  s.fwd2 = s.prep_in_fwd ? c % 2 : 0; c /= 2;
  s.stores_qkv1 = c % 2; c /= 2;
  s.stores_qkv2 = c % 2; c /= 2;
  const int tf = c % 3; c /= 3;                  // stores both expansions, the first, none
  s.stores_t1 = tf <= 1; s.stores_t2 = scale == 4 && tf == 0;
  s.tail_fwd = tf == 2 ? TAIL_FWD_X23_STREAM : TAIL_FWD_PLAIN;
  s.tail_bwd = c % 3 == 0 ? TAIL_BWD_PLAIN : (c % 3 == 1 ? TAIL_BWD_STORED : TAIL_BWD_X23_STREAM);
  return s;
}

struct Mode { int inference, local_norm, health; };
static const Mode MODES[6] = {{0, 0, 0}, {1, 0, 0}, {1, 8, 0}, {1, 64, 0}, {0, 0, 1}, {0, 0, 2}};

int main() {
  for (int dt : {M2T_F32, M2T_BF16})
    for (int scale : {2, 3, 4})
      for (int nb : {1, 2, 3, 8}) {
        for (const Mode& m : MODES)
          for (int c = 0; c < N_SCHED; ++c) {
            Plan p = make_plan(dt, scale, nb);
            p.s = sched(c, scale);
            p.g.inference = m.inference; p.g.local_norm = m.local_norm; p.g.health = m.health;
            p.resolve();
            check(p);
          }
        // the transitions: {inference, local_norm, health, schedule} after each step, then the fresh plan the last step must equal
        const int A = 0, U = 1;                  // two schedules: everything fused / nothing fused
        const int steps[5][4][4] = {{{1, 0, 0, A}, {0, 0, 0, A}, {-1}},
                                    {{0, 0, 2, A}, {0, 0, 0, A}, {-1}},
                                    {{0, 0, 1, A}, {0, 0, 1, U}, {0, 0, 0, U}, {0, 0, 0, A}},
                                    {{1, 0, 0, A}, {1, 64, 0, A}, {1, 0, 0, A}, {0, 0, 0, A}},
                                    {{1, 0, 0, A}, {1, 0, 0, U}, {0, 0, 0, U}, {0, 0, 2, U}}};
        const m2t_sched two[2] = {sched(1 + 2 * 2 + 6 * 1 + 48 * 2 + 144 * 2, scale), sched(12 + 24, scale)};
        for (const auto& tr : steps) {
          Plan p = make_plan(dt, scale, nb);
          const int* last = nullptr;
          for (const auto& st : tr) {
            if (st[0] < 0) break;
            p.g.inference = st[0]; p.g.local_norm = st[1]; p.g.health = st[2]; p.s = two[st[3]];
            p.resolve();
            check(p);
            last = st;
          }
          Plan f = make_plan(dt, scale, nb);
          f.g.inference = last[0]; f.g.local_norm = last[1]; f.g.health = last[2]; f.s = two[last[3]];
          f.resolve();
          EXPECT(same(p, f));
        }
      }
  if (failures) { fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
  printf("plan_layout_check: ok\n");
  return 0;
}
