// mcs::Fuse of host/mcs_multicol.hpp on a scripted map stand-in, the way an integrator binds
// cLocalMapping::SearchInNeighbors (rules 0 and 1) and cLoopClosing::SearchAndFuse (rule 2).
//   fuse_demo <dir> <rule> <bytes> <th> <th_low>
// <dir> holds the inputs as raw arrays (<name>.bin), written by tests/test_fuse_gpu.py.  Prints
// nFused per target, every action in execution order and the end state; the test compares them
// with the NumPy restatement.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../multicol-slam-annotation_amd/host/mcs_multicol.hpp"

static std::string g_dir;

template <class T>
static std::vector<T> load(const char* name, bool optional = false) {
  std::ifstream f(g_dir + "/" + name + ".bin", std::ios::binary);
  if (!f) {
    if (optional) return {};
    std::fprintf(stderr, "missing %s\n", name);
    std::exit(2);
  }
  std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<T> v(raw.size() / sizeof(T));
  std::memcpy(v.data(), raw.data(), v.size() * sizeof(T));
  return v;
}

// The map: isBad per point, and per keyframe mvpMapPoints plus which points observe it.  The
// observations of a point in a keyframe are the slots that hold it (as mcs_fuse_select assumes).
struct DemoMap : mcs::FuseMap {
  std::vector<uint8_t> bad;
  std::vector<std::vector<int32_t>> kp_mp;
  std::vector<std::vector<uint8_t>> in_kf;
  std::vector<uint8_t> new_desc;   // [n_mp][bytes] what ComputeDistinctiveDescriptors would give
  int bytes = 32;

  void state(int t, std::vector<uint8_t>& b, std::vector<uint8_t>& in, std::vector<int32_t>& slots) override {
    b = bad; in = in_kf[t]; slots = kp_mp[t];
  }
  void apply(int t, const std::vector<mcs::FuseAction>& actions, const std::vector<uint8_t>& b,
             const std::vector<uint8_t>& in, const std::vector<int32_t>& slots) override {
    bad = b; in_kf[t] = in; kp_mp[t] = slots;
    for (const mcs::FuseAction& a : actions) {
      std::printf("action %d %d %d %d %d\n", t, a.kind, a.query, a.keypoint, a.other);
      if (a.kind != MCS_FUSE_REPLACE) continue;
      // Replace in the other keyframes (src/cMapPoint.cpp:225-243): the replaced point's slots go
      // to the survivor, or are erased where the survivor already observes the keyframe
      const int32_t from = (*q_mp)[a.query], to = a.other;
      if (from == to) continue;
      for (size_t u = 0; u < kp_mp.size(); u++) {
        if ((int)u == t || !in_kf[u][from]) continue;
        for (size_t s = 0; s < kp_mp[u].size(); s++) {
          if (kp_mp[u][s] != from) continue;
          if (!in_kf[u][to]) { kp_mp[u][s] = to; in_kf[u][to] = 1; }
          else kp_mp[u][s] = -1;
        }
        in_kf[u][from] = 0;
      }
    }
  }
  void descriptor(int mp, uint8_t* desc, uint8_t*) override {
    std::memcpy(desc, &new_desc[(size_t)mp * bytes], bytes);
    std::printf("refresh %d\n", mp);
  }

  const std::vector<int32_t>* q_mp = nullptr;
};

int main(int argc, char** argv) {
  if (argc < 6) { std::fprintf(stderr, "usage: fuse_demo dir rule bytes th th_low\n"); return 2; }
  g_dir = argv[1];
  const int rule = std::atoi(argv[2]), bytes = std::atoi(argv[3]), th_low = std::atoi(argv[5]);
  const double th = std::atof(argv[4]);
  const std::vector<int32_t> dims = load<int32_t>("dims");   // n_cams, mirror_w, mirror_h, T, n_mp
  mcs::FuseRig rig;
  rig.n_cams = dims[0]; rig.mirror_w = dims[1]; rig.mirror_h = dims[2];
  rig.m_c = load<double>("m_c"); rig.cam = load<double>("cam"); rig.mirror = load<uint8_t>("mirror");
  rig.grid_params = load<double>("grid_params"); rig.scale = load<double>("scale");
  const int T = dims[3];
  std::vector<mcs::FuseKeyFrame> kfs(T);
  std::vector<const mcs::FuseKeyFrame*> targets;
  DemoMap map;
  map.n_mp = dims[4];
  map.bytes = bytes;
  map.bad = load<uint8_t>("mp_bad");
  map.new_desc = load<uint8_t>("new_desc");
  for (int t = 0; t < T; t++) {
    const std::string p = "t" + std::to_string(t) + "_";
    kfs[t].kp_xy = load<float>((p + "kp_xy").c_str());
    kfs[t].kp_octave = load<int32_t>((p + "kp_octave").c_str());
    kfs[t].kp_cam = load<int32_t>((p + "kp_cam").c_str());
    kfs[t].desc = load<uint8_t>((p + "desc").c_str());
    kfs[t].mask = load<uint8_t>((p + "mask").c_str(), true);
    kfs[t].rays = load<double>((p + "rays").c_str());
    const std::vector<double> m = load<double>((p + "m_t").c_str());
    if (rule == 2) mcs::FuseSim3ToMt(load<double>((p + "scw").c_str()).data(), kfs[t].m_t);
    else std::memcpy(kfs[t].m_t, m.data(), sizeof(kfs[t].m_t));
    map.kp_mp.push_back(load<int32_t>((p + "kp_mp").c_str()));
    map.in_kf.push_back(load<uint8_t>((p + "in_kf").c_str()));
    targets.push_back(&kfs[t]);
    for (int k = 0; k < 16; k++) std::printf("%s%.17g", k ? " " : "m_t ", kfs[t].m_t[k]);
    std::printf("\n");
  }
  mcs::FusePoints pts;
  pts.mp = load<int32_t>("q_mp"); pts.pos = load<double>("q_pos"); pts.dist = load<double>("q_dist");
  pts.desc = load<uint8_t>("q_desc"); pts.mask = load<uint8_t>("q_mask", true); pts.rays = load<double>("q_rays");
  const std::vector<double> cur = load<double>("q_m_t");
  std::memcpy(pts.cur_m_t, cur.data(), sizeof(pts.cur_m_t));
  map.q_mp = &pts.mp;
  std::vector<int> nf;
  try {
    nf = mcs::Fuse(rule, rig, targets, pts, bytes, th, th_low, map);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  for (int t = 0; t < T; t++) std::printf("nfused %d %d\n", t, nf[t]);
  std::printf("bad");
  for (uint8_t b : map.bad) std::printf(" %d", b);
  std::printf("\n");
  for (int t = 0; t < T; t++) {
    std::printf("slots %d", t);
    for (int32_t m : map.kp_mp[t]) std::printf(" %d", m);
    std::printf("\n");
  }
  return 0;
}
