// svr_dof_taps.h — the depth-of-field pass's 49 taps on the unit disc: the centre, then three rings
// j = 1, 2, 3 of 8j taps at radius j / 3 and angles 2 pi (i + (j even ? 0.5 : 0)) / (8j), i ascending.  Computed in fp64
// ((j / 3.0) * cos(a), (j / 3.0) * sin(a) with a = (2.0 * pi) * (i + turn) / (8j), a component below 2^-40 in magnitude
// being the exact 0 it stands for) and rounded once to fp32.  tests/native/dof_ref.cpp holds the same values, and
// tests/test_dof_ref.py regenerates them from the formula and compares the bits.
// Data only, as svr_ambient_tables.h: the including file says where the table lives.
#pragma once

#ifndef SVR_DOF_TABLE
#define SVR_DOF_TABLE static const
#endif

#define SVR_DOF_TAPS 49

SVR_DOF_TABLE float SVR_DOF_TAP[SVR_DOF_TAPS][2] = {
    {0x0.0p+0f, 0x0.0p+0f},
    // ring 1
    {0x1.555556p-2f, 0x0.0p+0f},
    {0x1.e2b7dep-3f, 0x1.e2b7dep-3f},
    {0x0.0p+0f, 0x1.555556p-2f},
    {-0x1.e2b7dep-3f, 0x1.e2b7dep-3f},
    {-0x1.555556p-2f, 0x0.0p+0f},
    {-0x1.e2b7dep-3f, -0x1.e2b7dep-3f},
    {0x0.0p+0f, -0x1.555556p-2f},
    {0x1.e2b7dep-3f, -0x1.e2b7dep-3f},
    // ring 2, turned by half a step
    {0x1.4ec654p-1f, 0x1.0a5d02p-3f},
    {0x1.1bceecp-1f, 0x1.7b44fp-2f},
    {0x1.7b44fp-2f, 0x1.1bceecp-1f},
    {0x1.0a5d02p-3f, 0x1.4ec654p-1f},
    {-0x1.0a5d02p-3f, 0x1.4ec654p-1f},
    {-0x1.7b44fp-2f, 0x1.1bceecp-1f},
    {-0x1.1bceecp-1f, 0x1.7b44fp-2f},
    {-0x1.4ec654p-1f, 0x1.0a5d02p-3f},
    {-0x1.4ec654p-1f, -0x1.0a5d02p-3f},
    {-0x1.1bceecp-1f, -0x1.7b44fp-2f},
    {-0x1.7b44fp-2f, -0x1.1bceecp-1f},
    {-0x1.0a5d02p-3f, -0x1.4ec654p-1f},
    {0x1.0a5d02p-3f, -0x1.4ec654p-1f},
    {0x1.7b44fp-2f, -0x1.1bceecp-1f},
    {0x1.1bceecp-1f, -0x1.7b44fp-2f},
    {0x1.4ec654p-1f, -0x1.0a5d02p-3f},
    // ring 3
    {0x1.0p+0f, 0x0.0p+0f},
    {0x1.ee8dd4p-1f, 0x1.0907dcp-2f},
    {0x1.bb67aep-1f, 0x1.0p-1f},
    {0x1.6a09e6p-1f, 0x1.6a09e6p-1f},
    {0x1.0p-1f, 0x1.bb67aep-1f},
    {0x1.0907dcp-2f, 0x1.ee8dd4p-1f},
    {0x0.0p+0f, 0x1.0p+0f},
    {-0x1.0907dcp-2f, 0x1.ee8dd4p-1f},
    {-0x1.0p-1f, 0x1.bb67aep-1f},
    {-0x1.6a09e6p-1f, 0x1.6a09e6p-1f},
    {-0x1.bb67aep-1f, 0x1.0p-1f},
    {-0x1.ee8dd4p-1f, 0x1.0907dcp-2f},
    {-0x1.0p+0f, 0x0.0p+0f},
    {-0x1.ee8dd4p-1f, -0x1.0907dcp-2f},
    {-0x1.bb67aep-1f, -0x1.0p-1f},
    {-0x1.6a09e6p-1f, -0x1.6a09e6p-1f},
    {-0x1.0p-1f, -0x1.bb67aep-1f},
    {-0x1.0907dcp-2f, -0x1.ee8dd4p-1f},
    {0x0.0p+0f, -0x1.0p+0f},
    {0x1.0907dcp-2f, -0x1.ee8dd4p-1f},
    {0x1.0p-1f, -0x1.bb67aep-1f},
    {0x1.6a09e6p-1f, -0x1.6a09e6p-1f},
    {0x1.bb67aep-1f, -0x1.0p-1f},
    {0x1.ee8dd4p-1f, -0x1.0907dcp-2f},
};
