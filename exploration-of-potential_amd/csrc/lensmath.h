// ep24 - the Kannala-Brandt polynomial and its inversion, shared by the lens maps (lens.hip) and the evaluator's distortion
// zones (evalstrata.hip).  All double, every operation rounded on its own (-ffp-contract=off); ep24.lens.LensModel.thetad /
// newton are the same arithmetic on the host.
#pragma once

// thetad(th) = th * (1 + k1 th^2 + k2 th^4 + k3 th^6 + k4 th^8), Horner in th^2
__host__ __device__ __forceinline__ double lens_thetad(double th, double k1, double k2, double k3, double k4) {
    const double t2 = th * th;
    return th * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))));
}

// Newton on thetad(th) = td from th = td, a fixed 12 steps, clamped to [0, tmax] after each (fmin / fmax also swallow a step that
// is not a number)
__device__ __forceinline__ double lens_newton(double td, double k1, double k2, double k3, double k4, double tmax) {
    double th = td;
#pragma unroll 1
    for (int it = 0; it < 12; ++it) {
        const double t2 = th * th;
        const double f = th * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))) - td;
        const double fp = 1.0 + t2 * (3.0 * k1 + t2 * (5.0 * k2 + t2 * (7.0 * k3 + t2 * (9.0 * k4))));
        th = th - f / fp;
        th = fmin(fmax(th, 0.0), tmax);
    }
    return th;
}
