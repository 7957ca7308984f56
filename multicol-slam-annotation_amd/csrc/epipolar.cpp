// The epipolar geometry of a keyframe pair on the host (C-ABI of include/mcs_matcher.h): the
// ComputeE table of a rig and CheckDistEpipolarLine.  Plain C++: no device.  Tiny 3x3 / 4x4
// math, nothing here is worth a launch; the functions are frm:: of omni_geom.hpp, the ones the
// kernels of tri_search.hip and fuse.hip call.
//
// ComputeE per camera pair (src/misc.cpp:72-86) as SearchForTriangulationRaw builds its Es table
// (src/cORBmatcher.cpp:985-998): Es[i][j] = ComputeE(KF1.Get_MtMc_inv(i), KF2.Get_MtMc(j)), with
// MtMc = cayley2hom(M_t) * cayley2hom(M_c) and MtMc_inv = cConverter::invMat(MtMc)
// (cMultiCamSys_::Set_M_t_from_min, src/cam_system_omni.cpp:170-183).
#include "common.hpp"
#include "omni_geom.hpp"
#include "../../include/mcs_matcher.h"

using namespace mcs;

// E [ncams][ncams][9] from the 4x4 poses T1, T2 and the rig's M_c: HOM = 16 doubles per camera
// (m_c as given), else mc [ncams][6] minimal, each made a 4x4 by cayley2hom where it is used
template <bool HOM>
static void compute_e_table(const double* T1, const double* T2, const double* mc, int ncams, double* E) {
  double Mc[16], R[9], t[3], Ri[9], ti[3];
  auto m_c = [&](int c) -> const double* {
    if (HOM) return mc + 16 * c;
    frm::cayley2hom(mc + 6 * c, Mc);
    return Mc;
  };
  for (int i = 0; i < ncams; i++) {
    frm::mtmc44(T1, m_c(i), R, t);
    frm::inv_rt(R, t, Ri, ti);
    for (int j = 0; j < ncams; j++) {
      frm::mtmc44(T2, m_c(j), R, t);
      frm::compute_e(Ri, ti, R, t, E + 9 * ((size_t)i * ncams + j));
    }
  }
}

extern "C" {

int mcs_compute_e_rig(const double* mt1, const double* mt2, const double* mc, int32_t ncams,
                      double* E) {
  if (!mt1 || !mt2 || !mc || !E || ncams <= 0) { set_error("compute_e_rig: bad arguments"); return MCS_ERR_ARG; }
  double T1[16], T2[16];
  frm::cayley2hom(mt1, T1);
  frm::cayley2hom(mt2, T2);
  compute_e_table<false>(T1, T2, mc, ncams, E);
  return MCS_OK;
}

int mcs_compute_e_rig_hom(const double* m_t1, const double* m_t2, const double* m_c, int32_t ncams,
                          double* E) {
  if (!m_t1 || !m_t2 || !m_c || !E || ncams <= 0) { set_error("compute_e_rig_hom: bad arguments"); return MCS_ERR_ARG; }
  compute_e_table<true>(m_t1, m_t2, m_c, ncams, E);
  return MCS_OK;
}

int mcs_check_dist_epipolar_line(const double* ray1, const double* ray2, const double* E12,
                                 double thresh) {
  if (!ray1 || !ray2 || !E12) { set_error("check_dist_epipolar_line: null argument"); return MCS_ERR_ARG; }
  return frm::epi_check(ray1, ray2, E12, thresh) ? 1 : 0;
}

}  // extern "C"
