// The one polygon-membership rule of libfusg: cv::fillPoly at shift 0 = the 8-connected outline drawn left to right
// (LineIterator) + the even-odd scanline interior with 16.16 fixed-point edge crossings, x1 = ceil(crossing),
// x2 = floor(next crossing) (drawing.cpp CollectPolyEdges / FillEdgeCollection).  Used by fill_poly_planes_kernel
// (cvops.hip: get_planes) and plane_visibility_kernel (render.hip: compute_visibility's areas); neither keeps a copy.
#pragma once

namespace fusg {

constexpr int MAXV = 8;                  // vertices per polygon

__device__ __forceinline__ bool on_line(int x, int y, int x0, int y0, int x1, int y1) {
    if (x1 < x0) { int t = x0; x0 = x1; x1 = t; t = y0; y0 = y1; y1 = t; }
    const int dx = x1 - x0, dyv = y1 - y0, dy = dyv < 0 ? -dyv : dyv, sy = dyv >= 0 ? 1 : -1;
    if (dx >= dy) {
        const int k = x - x0;
        if (k < 0 || k > dx) return false;
        const int yy = y0 + sy * (dx ? (int)((2L * dy * k + dx - 1) / (2L * dx)) : 0);
        return yy == y;
    }
    const int k = (y - y0) * sy;
    if (k < 0 || k > dy) return false;
    return x0 + (int)((2L * dx * k + dy - 1) / (2L * dy)) == x;
}

// pixel (x, y) inside or on the outline of the polygon of nv (<= MAXV) vertices (px[i], py[i])
__device__ __forceinline__ bool poly_inside(int x, int y, int nv, const int* px, const int* py) {
    bool in = false;
    long xs[MAXV];
    int nx = 0;
    for (int i = 0; i < nv; ++i) {
        const int j = i == 0 ? nv - 1 : i - 1;
        const int ax = px[j], ay = py[j], bx = px[i], by = py[i];
        in = in || on_line(x, y, ax, ay, bx, by);
        if (ay == by) continue;
        const int y0 = ay < by ? ay : by, y1 = ay < by ? by : ay, xa = ay < by ? ax : bx;
        if (y < y0 || y >= y1) continue;
        const long num = ((long)bx - ax) << 16, den = (long)by - ay;
        const long dxf = num / den;                                    // C++ integer division truncates toward zero
        const long xc = ((long)xa << 16) + dxf * (y - y0);
        int k = nx++;
        while (k > 0 && xs[k - 1] > xc) { xs[k] = xs[k - 1]; --k; }   // insertion sort (<= 8 crossings)
        xs[k] = xc;
    }
    for (int k = 0; k + 1 < nx; k += 2) {
        const long x1 = (xs[k] + 65535) >> 16, x2 = xs[k + 1] >> 16;
        in = in || (x >= x1 && x <= x2);
    }
    return in;
}

}  // namespace fusg
