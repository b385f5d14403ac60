// svr_ambient_tables.h — the literals of the ambient pass's tap pattern.  Data only: included by
// k_ambient.hip and by tests/native/ambient_ref.cpp, so both read the same bits.
//   SVR_AMBIENT_D[k]  the direction of tap k: the eight unit vectors at multiples of 45 degrees.
//   SVR_AMBIENT_R[j]  (cos, sin) of j * 45 / 16 degrees, rounded to fp32: sixteen rotations that fill the gap between two
//                     directions; a pixel takes j = (py & 3) * 4 + (px & 3).
// tests/test_ambient_ref.py states the properties: every rotated direction is within 2 ulp of unit length, and the
// sixteen rotations are distinct.
#pragma once

#ifndef SVR_AMBIENT_TABLE
#define SVR_AMBIENT_TABLE static const
#endif

SVR_AMBIENT_TABLE float SVR_AMBIENT_D[8][2] = {
    {1.0f, 0.0f},  {0.70710678f, 0.70710678f},   {0.0f, 1.0f},  {-0.70710678f, 0.70710678f},
    {-1.0f, 0.0f}, {-0.70710678f, -0.70710678f}, {0.0f, -1.0f}, {0.70710678f, -0.70710678f},
};

SVR_AMBIENT_TABLE float SVR_AMBIENT_R[16][2] = {
    {1.0f, 0.0f},
    {0.99879545f, 0.049067676f},
    {0.9951847f, 0.09801714f},
    {0.9891765f, 0.14673047f},
    {0.98078525f, 0.19509032f},
    {0.97003126f, 0.24298018f},
    {0.95694035f, 0.29028466f},
    {0.94154406f, 0.33688986f},
    {0.9238795f, 0.38268343f},
    {0.9039893f, 0.42755508f},
    {0.8819213f, 0.47139674f},
    {0.8577286f, 0.51410276f},
    {0.8314696f, 0.55557024f},
    {0.8032075f, 0.5956993f},
    {0.77301043f, 0.6343933f},
    {0.7409511f, 0.671559f},
};
