// request_policy_host.cpp -- walks the cells of tests/request_policy_cells.py through apply_requests for every row of
// kRequestPolicies, without a device (built by tests/test_request_policy_host.py with the host compiler, beside
// csrc/requests.cpp).  One line per cell:
//   <symbol> <byband> <mask> <jacobian> <aerosol> <active> <status> <extras or message>
// where an accepted cell (status 0) lists the fields of SolverExtras that were set.
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
// the rows whose entries have a *_gpt twin
static const PolicyRow kTwins[] = {kRowLwNoscat, kRowLwNoscatPlanck, kRowLw1rescl, kRowLw2stream, kRowSw2stream,
                                   kRowSwNoscat};

static ArmedRequests arm(bool sw, int byband, int mask, int jacobian, int aerosol, int active)
{
  static float f[4];
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
  return rq;
}

static void walk(const RequestPolicy &p, bool gpt)
{
  const bool sw = std::strncmp(p.entry, "sw_", 3) == 0;
  for (int b = 0; b < 3; b++)
    for (int m = 0; m < 4; m++)
      for (int j = 0; j < 4; j++)
        for (int a = 0; a < 4; a++)
          for (int n = 0; n < 3; n++) {
            if (m == 2 && b != 1) continue;
            SolverExtras ex;
            g_message.clear();
            const int rc = apply_requests(p, arm(sw, b, m, j, a, n), {NGPT, NBND, NLAY, NCOL, gpt}, ex);
            std::printf("%s%s %d %d %d %d %d %d ", p.entry, gpt ? "_gpt" : "", b, m, j, a, n, rc);
            if (rc)
              std::printf("%s\n", g_message.c_str());
            else
              std::printf("%s%s%s%s%s%s%s%s\n", ex.byband() ? "byband," : "", ex.mask_bits ? "mask_bits," : "",
                          ex.jac_up ? "jac_up," : "", ex.sfc_jac ? "sfc_jac," : "", ex.aer_tau ? "aer_tau," : "",
                          ex.aer_ssa ? "aer_ssa," : "", ex.aer_g ? "aer_g," : "", ex.nact ? "nact," : "");
          }
}

int main()
{
  for (int r = 0; r < kNumPolicyRows; r++) walk(kRequestPolicies[r], false);
  for (PolicyRow r : kTwins) walk(kRequestPolicies[r], true);
  return 0;
}
