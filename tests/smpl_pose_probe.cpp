// smpl_pose_probe.cpp -- thin C interface over the way back in uhc_amd/csrc/uhc_smpl_convert.h (qpos rows -> SMPL poses, and the 6D rows) for
// tests/test_smpl_pose_cpu.py: built with the host compiler, no HIP.  The header's per-joint pieces are what the device kernels (uhc_smpl.hip) compute with, one
// lane per row and joint; here the joints are the header's own loops.
#include "uhc_smpl_convert.h"

#define PROBE_API extern "C" __attribute__((visibility("default")))

// qpos [n] rows of `stride` doubles (hinge rows, or ball-joint rows with ball != 0), offset [3] or NULL, slot_of_joint [24]
// -> pose_aa [n][72], trans [n][3], full_6d [n][147] (NULL: not written); returns the number of bad rows (NaN throughout)
PROBE_API long uhc_pose_probe_rows(const double* qpos, long stride, int ball, const double* offset, const int* slot_of_joint, long n, double* pose_aa, double* trans,
                                   double* full_6d) {
    long bad = 0;
    for (long r = 0; r < n; r++)
        bad += uhc_sc_pose_row_serial(qpos + stride * r, ball, offset, slot_of_joint, pose_aa ? pose_aa + 72 * r : nullptr, trans ? trans + 3 * r : nullptr,
                                      full_6d ? full_6d + UHC_SC_N6D * r : nullptr);
    return bad;
}

// full_6d [n][147], offset [3] or NULL -> qpos [n][76] and / or qpos_quat [n][99] (NULL: not written)
PROBE_API void uhc_pose_probe_rows6d(const double* full_6d, const double* offset, const int* slot_of_joint, long n, double* qpos, double* qpos_quat) {
    for (long f = 0; f < n; f++)
        uhc_sc_row6d_serial(full_6d + UHC_SC_N6D * f, offset, slot_of_joint, qpos ? qpos + UHC_SC_NQ * f : nullptr, qpos_quat ? qpos_quat + UHC_SC_NQ_QUAT * f : nullptr);
}

// one quaternion (x, y, z, w), taken as it is -> its rotation vector
PROBE_API void uhc_pose_probe_rotvec(const double* xyzw, double* rotvec) {
    const UhcScV3 r = uhc_sc_quat_rotvec({xyzw[0], xyzw[1], xyzw[2], xyzw[3]});
    rotvec[0] = r.x, rotvec[1] = r.y, rotvec[2] = r.z;
}
