// smpl_convert_probe.cpp -- thin C interface over uhc_amd/csrc/uhc_smpl_convert.h for tests/test_smpl_convert_cpu.py: built with the host compiler, no HIP.
// The header's per-joint pieces are what the device kernel (uhc_smpl.hip) computes with, one lane per frame and joint; here the joints are the header's own loop.
#include "uhc_smpl_convert.h"

#define PROBE_API extern "C" __attribute__((visibility("default")))

// pose [n][72], trans [n][3] or NULL, offset [3] or NULL, slot_of_joint [24] -> qpos [n][76] and / or qpos_quat [n][99] (NULL: not written)
PROBE_API void uhc_smpl_probe_rows(const double* pose, const double* trans, const double* offset, const int* slot_of_joint, long n, double* qpos, double* qpos_quat) {
    for (long f = 0; f < n; f++)
        uhc_sc_row_serial(pose + 72 * f, trans ? trans + 3 * f : nullptr, offset, slot_of_joint, qpos ? qpos + UHC_SC_NQ * f : nullptr,
                          qpos_quat ? qpos_quat + UHC_SC_NQ_QUAT * f : nullptr);
}

// one rotation vector -> its intrinsic ZYX Euler triple (Z, Y, X)
PROBE_API void uhc_smpl_probe_euler(const double* rotvec, double* zyx) {
    const UhcScEuler e = uhc_sc_quat_euler_zyx(uhc_sc_rotvec_quat(rotvec[0], rotvec[1], rotvec[2]));
    zyx[0] = e.Z, zyx[1] = e.Y, zyx[2] = e.X;
}
