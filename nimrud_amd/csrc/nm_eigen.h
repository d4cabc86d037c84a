// nm_eigen.h - the fp64 3x3 symmetric eigen-solve and the eigenvector construction on top of it (device only).
// shared by the feature kernels (nm_features.hip: normal_out) and the segment table (nm_segments.hip: normal and axis).
// nothing here fuses a multiply-add: both files are compiled with -ffp-contract=off.
#pragma once

#if defined(__HIPCC__)

// ---- 3x3 symmetric eigenvalues, fp64, non-iterative ------------------------------------------------
// eigenvalues of [[a00,a01,a02],[a01,a11,a12],[a02,a12,a22]] in descending order.
// the trigonometric solution of the characteristic cubic is accurate only for the eigenvalue that is
// well separated from the other two (the other two lose sqrt(eps) when they nearly coincide, which
// is the normal case here: collinear and coplanar lattice neighborhoods have exact double roots).
// so: take the separated eigenvalue from the cubic, form its eigenvector from the cross products of
// the rows of (A - lambda*I), deflate A onto the orthogonal complement and solve the remaining
// symmetric 2x2 in closed form (hypot form, no cancellation).  all three eigenvalues then carry an
// absolute error of a few ulp of ||A||, like LAPACK's.
__device__ __forceinline__ void nm_eig3(double a00, double a01, double a02, double a11, double a12,
                                        double a22, double& l0, double& l1, double& l2)
{
    const double p1 = a01 * a01 + a02 * a02 + a12 * a12;
    const double q = (a00 + a11 + a22) * (1.0 / 3.0);
    const double b00 = a00 - q, b11 = a11 - q, b22 = a22 - q;
    const double p2 = b00 * b00 + b11 * b11 + b22 * b22 + 2.0 * p1;
    if (!(p2 > 0.0)) {
        l0 = l1 = l2 = q;
        return;
    }
    const double p = sqrt(p2 * (1.0 / 6.0));
    const double inv = 1.0 / p;
    const double c00 = b00 * inv, c11 = b11 * inv, c22 = b22 * inv;
    const double c01 = a01 * inv, c02 = a02 * inv, c12 = a12 * inv;
    const double det = c00 * (c11 * c22 - c12 * c12) - c01 * (c01 * c22 - c12 * c02) +
                       c02 * (c01 * c12 - c11 * c02);
    const double r = fmin(fmax(det * 0.5, -1.0), 1.0);
    // with x = (lambda - q)/p the characteristic cubic is x^3 - 3x - 2r = 0, roots 2cos(phi + 2k*pi/3).
    // r >= 0: the largest root (in [sqrt3, 2]) is the separated one; r < 0: the smallest (mirror
    // image).  Newton from x = 2 descends monotonically onto that root; f' >= 6 there, so it is
    // quadratic and well conditioned.  (this replaces acos/cos: the fp64 library versions cost ~100
    // registers, i.e. two waves of occupancy.)  the approximate reciprocal only perturbs the step.
    const bool top = r >= 0.0;
    const double ra = fabs(r);
    double x = 2.0;
#pragma unroll
    for (int it = 0; it < 7; ++it) {
        const double x2 = x * x;
        const double f = x * (x2 - 3.0) - 2.0 * ra;
        const double fp = 3.0 * x2 - 3.0;
        x = x - f * __builtin_amdgcn_rcp(fp);
    }
    const double lam = top ? q + p * x : q - p * x;

    // eigenvector of lam: the cross product of two rows of (A - lam*I) with the largest norm
    const double m00 = a00 - lam, m11 = a11 - lam, m22 = a22 - lam;
    double x0 = a01 * a12 - a02 * m11, y0 = a02 * a01 - m00 * a12, z0 = m00 * m11 - a01 * a01;  // r0 x r1
    double x1 = a01 * m22 - a02 * a12, y1 = a02 * a02 - m00 * m22, z1 = m00 * a12 - a01 * a02;  // r0 x r2
    double x2 = m11 * m22 - a12 * a12, y2 = a12 * a02 - a01 * m22, z2 = a01 * a12 - m11 * a02;  // r1 x r2
    double n0 = x0 * x0 + y0 * y0 + z0 * z0;
    double n1 = x1 * x1 + y1 * y1 + z1 * z1;
    double n2 = x2 * x2 + y2 * y2 + z2 * z2;
    double vx = x0, vy = y0, vz = z0, nn = n0;
    if (n1 > nn) { vx = x1; vy = y1; vz = z1; nn = n1; }
    if (n2 > nn) { vx = x2; vy = y2; vz = z2; nn = n2; }
    if (!(nn > 0.0)) {
        // (A - lam*I) has rank <= 1: the other two eigenvalues coincide; they share what is left of
        // the trace
        const double rest = 0.5 * (3.0 * q - lam);
        if (top) {
            l0 = lam; l1 = rest; l2 = rest;
        } else {
            l0 = rest; l1 = rest; l2 = lam;
        }
        return;
    }
    const double vn = 1.0 / sqrt(nn);
    vx *= vn; vy *= vn; vz *= vn;
    // orthonormal basis (u, w) of the complement of v
    double ux, uy, uz;
    if (fabs(vx) > fabs(vy)) {
        const double s = 1.0 / sqrt(vx * vx + vz * vz);
        ux = -vz * s; uy = 0.0; uz = vx * s;
    } else {
        const double s = 1.0 / sqrt(vy * vy + vz * vz);
        ux = 0.0; uy = vz * s; uz = -vy * s;
    }
    const double wx = vy * uz - vz * uy, wy = vz * ux - vx * uz, wz = vx * uy - vy * ux;
    // 2x2 block of A in that basis
    const double aux = a00 * ux + a01 * uy + a02 * uz, auy = a01 * ux + a11 * uy + a12 * uz,
                 auz = a02 * ux + a12 * uy + a22 * uz;
    const double awx = a00 * wx + a01 * wy + a02 * wz, awy = a01 * wx + a11 * wy + a12 * wz,
                 awz = a02 * wx + a12 * wy + a22 * wz;
    const double e00 = ux * aux + uy * auy + uz * auz;
    const double e01 = ux * awx + uy * awy + uz * awz;
    const double e11 = wx * awx + wy * awy + wz * awz;
    const double mid = 0.5 * (e00 + e11), hd = 0.5 * (e00 - e11);
    const double rad = sqrt(hd * hd + e01 * e01);
    const double hi = mid + rad, lo = mid - rad;
    if (top) {
        l0 = lam; l1 = hi; l2 = lo;
    } else {
        l0 = hi; l1 = lo; l2 = lam;
    }
}

// unit eigenvector of the eigenvalue `lam` of a symmetric matrix scaled to unit size (trace 1): the largest cross
// product of two rows of A - lam I; where that matrix has rank <= 1 (lam is not simple) some unit vector of the
// eigenspace.  (gx, gy, gz) = -1 mirrors an axis back into the true frame.  sign: last non-zero of (x, y, z) positive.
__device__ __forceinline__ void nm_unit_eigenvector(double a00, double a01, double a02, double a11, double a12,
                                                    double a22, double lam, double gx, double gy, double gz,
                                                    double* __restrict__ v)
{
    const double m00 = a00 - lam, m11 = a11 - lam, m22 = a22 - lam;
    double x0 = a01 * a12 - a02 * m11, y0 = a02 * a01 - m00 * a12, z0 = m00 * m11 - a01 * a01;
    double x1 = a01 * m22 - a02 * a12, y1 = a02 * a02 - m00 * m22, z1 = m00 * a12 - a01 * a02;
    double x2 = m11 * m22 - a12 * a12, y2 = a12 * a02 - a01 * m22, z2 = a01 * a12 - m11 * a02;
    const double n0 = x0 * x0 + y0 * y0 + z0 * z0, n1 = x1 * x1 + y1 * y1 + z1 * z1,
                 n2 = x2 * x2 + y2 * y2 + z2 * z2;
    double vx = x0, vy = y0, vz = z0, nn = n0;
    if (n1 > nn) { vx = x1; vy = y1; vz = z1; nn = n1; }
    if (n2 > nn) { vx = x2; vy = y2; vz = z2; nn = n2; }
    if (!(nn > 0.0)) {
        // A - lambda I has rank <= 1: every direction orthogonal to its one row direction will do
        vx = 0.0; vy = 0.0; vz = 1.0;
        const double r0 = m00 * m00 + a01 * a01 + a02 * a02, r1 = a01 * a01 + m11 * m11 + a12 * a12,
                     r2 = a02 * a02 + a12 * a12 + m22 * m22;
        double rx = m00, ry = a01, rz = a02, rr = r0;
        if (r1 > rr) { rx = a01; ry = m11; rz = a12; rr = r1; }
        if (r2 > rr) { rx = a02; ry = a12; rz = m22; rr = r2; }
        if (rr > 0.0) {
            // a vector orthogonal to (rx, ry, rz)
            if (fabs(rx) > fabs(rz)) { vx = -ry; vy = rx; vz = 0.0; }
            else { vx = 0.0; vy = -rz; vz = ry; }
            if (vx == 0.0 && vy == 0.0 && vz == 0.0) { vx = 1.0; }
        }
        nn = vx * vx + vy * vy + vz * vz;
    }
    const double s = 1.0 / sqrt(nn);
    vx *= s * gx;
    vy *= s * gy;
    vz *= s * gz;
    // "last non-zero component positive": a component that is zero in exact arithmetic (the z of a wall's normal)
    // comes out as rounding noise of either sign, some 1e-16 over the eigenvalue gap, and must not decide the
    // orientation - below 1e-12, the accuracy of the vector itself, a component counts as zero
    const double tiny = 1e-12;
    const bool flip = vz < -tiny || (!(vz > tiny) && (vy < -tiny || (!(vy > tiny) && vx < 0.0)));
    v[0] = flip ? -vx : vx;
    v[1] = flip ? -vy : vy;
    v[2] = flip ? -vz : vz;
}

// unit eigenvector of the smallest eigenvalue of n S2 - S1 S1^T (the plane normal of the neighborhood), in
// the true frame (gx, gy, gz = -1 where the moments were taken mirrored), last non-zero of (x, y, z) positive.
// the smallest eigenvalue comes from the robust solver; its eigenvector is the largest cross product of
// two rows of A - lambda I, on the matrix scaled to unit size.
__device__ __forceinline__ void nm_normal_from_moments(
    double n, double sx, double sy, double sz, double sxx, double sxy, double sxz, double syy,
    double syz, double szz, double gx, double gy, double gz, double* __restrict__ v)
{
    v[0] = v[1] = v[2] = 0.0;
    if (n < 3.0) return;
    double a00 = n * sxx - sx * sx, a01 = n * sxy - sx * sy, a02 = n * sxz - sx * sz;
    double a11 = n * syy - sy * sy, a12 = n * syz - sy * sz, a22 = n * szz - sz * sz;
    const double tr = a00 + a11 + a22;
    if (!(tr > 0.0)) return;
    const double inv = 1.0 / tr;
    a00 *= inv; a01 *= inv; a02 *= inv; a11 *= inv; a12 *= inv; a22 *= inv;
    double l0, l1, l2;
    nm_eig3(a00, a01, a02, a11, a12, a22, l0, l1, l2);
    nm_unit_eigenvector(a00, a01, a02, a11, a12, a22, l2, gx, gy, gz, v);
}

#endif  // __HIPCC__
