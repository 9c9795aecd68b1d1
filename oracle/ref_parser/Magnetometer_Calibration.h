// Stand-in for the reference's Eigen / CUDA magnetometer calibration: never calibrated, so every
// phase-1 message reaches setValues, which records its arguments ("C set x y z"); CorrectValues does
// nothing, as in the reference, whose body is commented out.
#pragma once
#include <cstdio>

extern FILE *ref_trace;

class Magnetometer_Calibration
{
public:
	void setValues(double x, double y, double z) { std::fprintf(ref_trace, "C set %a %a %a\n", x, y, z); }
	bool MagnetometerCalibrated() { return false; }
	void CorrectValues(double &, double &, double &) {}
};
