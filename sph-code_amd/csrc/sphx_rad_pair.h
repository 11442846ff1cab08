// sphx_rad_pair.h - the (particle, ray) term of rad_heating's column sum (nsc:927-928), written once for the column
// kernel's two modes.
#pragma once

#define SPHX_RAD_C2 (3.0 * 3.141592653589793 / 80.0)     /* the reference's W6_constant = 3 pi / 80, nsc:48 (not 315/64 pi) */

// a.b by the same three operations wherever it is formed: a particle AT a ray's target gives (x - a).u == u.u bit for
// bit (the half-open end test leaves it out), one AT the source gives 0 (in)
__device__ __forceinline__ double rad_dot(double ax, double ay, double az, double bx, double by, double bz) {
    return fma(az, bz, fma(ay, by, ax * bx));
}

// w_p where particle p blocks the ray from a along u, else 0.  The reference divides, d2 = |(x - a) x u|^2 / |u|^2 < h^2;
// this compares |(x - a) x u|^2 < h^2 |u|^2 - the same set wherever no pair sits within rounding of the edge.  A
// degenerate ray (u = 0) gives 0 < 0: nothing blocks it (the reference: d2 = NaN, NaN < h^2 is false).
// SEG: only a foot point between source and target counts, 0 <= (x - a).u < |u|^2.
template <bool SEG>
__device__ __forceinline__ double rad_pair(double px, double py, double pz, double h2, double w, double ax, double ay,
                                           double az, double ux, double uy, double uz, double uu) {
    const double dx = px - ax, dy = py - ay, dz = pz - az;
    const double cx = dy * uz - dz * uy, cy = dz * ux - dx * uz, cz = dx * uy - dy * ux;
    bool in = cx * cx + cy * cy + cz * cz < h2 * uu;
    if (SEG) {
        const double t = rad_dot(dx, dy, dz, ux, uy, uz);
        in = in && t >= 0.0 && t < uu;
    }
    return in ? w : 0.0;
}
