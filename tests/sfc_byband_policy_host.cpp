// sfc_byband_policy_host.cpp -- walks rrtmgpnn_solver_request_sfc_byband (off, armed, of another ncol, with limits past
// ngpt) against every cell of the five other request kinds (the cells of tests/request_policy_host.cpp) through
// apply_requests for every row of kRequestPolicies, without a device (built by tests/test_sfc_byband_host.py with the
// host compiler, beside csrc/requests.cpp).  One line per cell and state of the new request:
//   <entry> <byband> <mask> <jacobian> <aerosol> <active> <sfc> <status> <extras or message>
// sfc: 0 the member as ArmedRequests{} leaves it, 1 filled in but not armed, 2 armed, 3 armed with another ncol, 4 armed
// with limits past ngpt.  An accepted cell (status 0) lists the fields of SolverExtras that were set.
#include <cstdio>
#include <cstring>
#include <string>

#include "requests.hpp"

using namespace rrtmgpnn;

static std::string g_message;
int rrtmgpnn::fail(int code, const std::string &msg)
{
  g_message = msg;
  return code;
}

static const int NGPT = 4, NBND = 2, NLAY = 2, NCOL = 3;
static float f[4], up[NBND * (NCOL + 1)], dn[NBND * (NCOL + 1)], dir[NBND * (NCOL + 1)];

static ArmedRequests arm(bool sw, int byband, int mask, int jacobian, int aerosol, int active, int sfc)
{
  static uint32_t bits[4];
  static int word[1];
  ArmedRequests rq;
  if (byband) {
    const int lims[4] = {1, 2, 3, byband == 2 ? 5 : 4};
    rq.byband.armed = true;
    rq.byband.up = rq.byband.dn = rq.byband.dir = f;
    rq.byband.nbnd = NBND;
    std::memcpy(rq.byband.lims, lims, sizeof lims);
  }
  if (mask) rq.cloud_mask = {true, mask == 2, NGPT, NLAY, NCOL + (mask == 3), bits};
  if (jacobian) rq.jacobian = {true, NGPT, NLAY, NCOL + (jacobian == 3), jacobian == 2 ? nullptr : f, f};
  if (aerosol) {
    const float *sg = aerosol == 2 || (aerosol == 3 && sw) ? f : nullptr;
    rq.aerosol = {true, NBND, NLAY, NCOL + (aerosol == 3), f, sg, sg};
  }
  if (active) rq.active = {true, NCOL + (active == 2), word};
  if (sfc) {
    const int lims[4] = {1, 2, 3, sfc == 4 ? 5 : 4};
    rq.sfc_byband.armed = sfc > 1;
    rq.sfc_byband.up = up;
    rq.sfc_byband.dn = dn;
    rq.sfc_byband.dir = dir;
    rq.sfc_byband.nbnd = NBND;
    rq.sfc_byband.ncol = NCOL + (sfc == 3);
    std::memcpy(rq.sfc_byband.lims, lims, sizeof lims);
  }
  return rq;
}

static void walk(const RequestPolicy &p)
{
  const bool sw = std::strncmp(p.entry, "sw_", 3) == 0;
  for (int b = 0; b < 3; b++)
    for (int m = 0; m < 4; m++)
      for (int j = 0; j < 4; j++)
        for (int a = 0; a < 4; a++)
          for (int n = 0; n < 3; n++)
            for (int s = 0; s < 5; s++) {
              if (m == 2 && b != 1) continue;
              SolverExtras ex;
              g_message.clear();
              const int rc = apply_requests(p, arm(sw, b, m, j, a, n, s), {NGPT, NBND, NLAY, NCOL, false}, ex);
              std::printf("%s %d %d %d %d %d %d %d ", p.entry, b, m, j, a, n, s, rc);
              if (rc) {
                std::printf("%s\n", g_message.c_str());
                continue;
              }
              // the surface outputs are the request's own pointers and its limits, or nothing at all
              const bool whole = ex.sfc_bnd_up == up && ex.sfc_bnd_dn == dn && ex.sfc_bnd_dir == dir &&
                                 ex.sfc_bnd.nbnd == NBND && ex.sfc_bnd.lims[0] == 1 && ex.sfc_bnd.lims[1] == 2 &&
                                 ex.sfc_bnd.lims[2] == 3 && ex.sfc_bnd.lims[3] == 4;
              const bool none = !ex.sfc_byband() && ex.sfc_bnd.nbnd == 0;
              std::printf("%s%s%s%s%s%s%s%s%s\n", ex.byband() ? "byband," : "", ex.mask_bits ? "mask_bits," : "",
                          ex.jac_up ? "jac_up," : "", ex.sfc_jac ? "sfc_jac," : "", ex.aer_tau ? "aer_tau," : "",
                          ex.aer_ssa ? "aer_ssa," : "", ex.aer_g ? "aer_g," : "", ex.nact ? "nact," : "",
                          whole ? "sfc_bnd," : (none ? "" : "sfc_bnd_partly,"));
            }
}

int main()
{
  for (int r = 0; r < kNumPolicyRows; r++) walk(kRequestPolicies[r]);
  return 0;
}
