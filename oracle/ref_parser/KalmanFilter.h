// Stand-in for the reference's Eigen filter: computes nothing, records every call Parser.cpp makes
// ("K <call> <arguments>", doubles as %a, times in decimal) into the driver's trace.
#pragma once
#include <array>
#include <cstdio>
#include <map>
#include <string>

extern FILE *ref_trace;

class KalmanFilter
{
public:
	KalmanFilter() {}
	KalmanFilter(std::map<std::string, std::array<double, 3>> Values, long long timestamp)
	{
		const std::array<double, 3> &m = Values["mag0"], &a = Values["acc0"];
		std::fprintf(ref_trace, "K ctor %a %a %a %a %a %a %lld\n", m[0], m[1], m[2], a[0], a[1], a[2], timestamp);
	}
	void SetAngularVelocity(double w_x, double w_y, double w_z, long long timestamp)
	{
		std::fprintf(ref_trace, "K gyro %a %a %a %lld\n", w_x, w_y, w_z, timestamp);
	}
	void SetMagnetometerMeasurements(double m_x, double m_y, double m_z)
	{
		std::fprintf(ref_trace, "K mag %a %a %a\n", m_x, m_y, m_z);
	}
	void SetAccelerometerMeasurements(double a_x, double a_y, double a_z)
	{
		std::fprintf(ref_trace, "K acc %a %a %a\n", a_x, a_y, a_z);
	}
	void getXk_1(double *) {}
	void getRPY(double *) {}
	void UpdateLatestPreviousTime(long long Time) { std::fprintf(ref_trace, "K time %lld\n", Time); }
};
