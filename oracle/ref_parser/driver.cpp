// ref_parser: the reference server's own Parser (a staged copy of its Parser.cpp / InitialValues.cpp,
// compiled unchanged against the stand-in headers of this directory) fed with wire frames, and a trace
// of what it made of them.  TEST INFRASTRUCTURE ONLY: tests/golden/make_parser_golden.py runs it to
// produce tests/golden/parser.npz.
//
//   ref_parser TRACE < frames        (frames: whole 100-byte frames; TRACE: the trace file, default stderr;
//                                     the parser's own chatter goes to stdout)
//
// A frame is handled as the server handles a recv of 100 bytes (Server.cpp:84-97, Parser.cpp:357-363):
// the message is std::string(buf, 0, n) with buf a char* -- through strlen, so a NUL cuts it --, only a
// message starting with '#' is taken, without the '#', and ProcessString does the rest.  An exception of
// std::stod / std::stoll, which ends the real server, is recorded and the run goes on (ProcessString has
// changed nothing but `phase` by then).
//
// Trace, one line each (doubles as %a, integers in decimal):
//   F <frame> <message length> nohash|short|call     what became of the frame ('short': 30 characters or
//                                                    fewer after '#', Parser.cpp:14); after 'call' follow
//   K ... / C ...                                    the stand-ins' records of the calls made meanwhile,
//   R ok|threw                                       how ProcessString returned,
//   I a|m|g <x> <y> <z>                              the sample a phase-2 message added to a sensor's sums,
//   S <phase> <gyro_is_set> <acc_1_is_set> <mag_1_is_set>  <gyro x y z t>  <acc_0 ..>  <acc_1 ..>  <mag_0 ..>
//     <mag_1 ..>  <acc_count> <mag_count> <gyr_count>  <Acc_> <Mag_> <Gyr_> <Kalman_initialized>
//                                                    the parser's state after it;
//   E <avg_acc x y z> <avg_mag> <avg_gyr> <variance_acc> <variance_mag> <variance_gyr> <Acc_> <Mag_> <Gyr_>
//     <Kalman_initialized>                           once, at the end.
// Built with -fno-access-control, which is what lets this file call ProcessString and read the state.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>

#include "Parser.h"

FILE *ref_trace = stderr;

static Parser parser;  // static storage: the members the reference leaves uninitialised start as zero

static void put3(const std::array<double, 3> &v) { std::fprintf(ref_trace, " %a %a %a", v[0], v[1], v[2]); }
static void put3t(const std::array<double, 3> &v, long long t)
{
	put3(v);
	std::fprintf(ref_trace, " %lld", t);
}
static void sample(char name, InitialValues &iv, int before)
{
	// the arrays are freed once the last sample is in (InitialValues.cpp:30-34,70-72)
	if (iv.n != before && !iv.isCalibrated)
		std::fprintf(ref_trace, "I %c %a %a %a\n", name, iv.x[iv.n - 1], iv.y[iv.n - 1], iv.z[iv.n - 1]);
}

int main(int argc, char **argv)
{
	if (argc > 1 && !(ref_trace = std::fopen(argv[1], "w")))
	{
		std::perror(argv[1]);
		return 1;
	}
	Parser &p = parser;
	char *buf = (char *)std::calloc(101, 1);  // (the server's is 100 bytes: its strlen runs off the end)
	for (long frame = 0; std::fread(buf, 1, 100, stdin) == 100; ++frame)
	{
		std::string Measurement = std::string(buf, 0, 100);
		const unsigned long len = Measurement.size();
		if (Measurement[0] != '#')
		{
			std::fprintf(ref_trace, "F %ld %lu nohash\n", frame, len);
			continue;
		}
		Measurement = Measurement.substr(1, Measurement.size() - 1);
		if (!(Measurement.size() > 30))
		{
			std::fprintf(ref_trace, "F %ld %lu short\n", frame, len);
			p.ProcessString(Measurement);  // (only prints and remembers the string)
			continue;
		}
		std::fprintf(ref_trace, "F %ld %lu call\n", frame, len);
		const int na = p.init_acc.n, nm = p.init_mag.n, ng = p.init_gyro.n;
		bool threw = false;
		try
		{
			p.ProcessString(Measurement);
		}
		catch (const std::exception &)
		{
			threw = true;
		}
		std::fprintf(ref_trace, "R %s\n", threw ? "threw" : "ok");
		sample('a', p.init_acc, na);
		sample('m', p.init_mag, nm);
		sample('g', p.init_gyro, ng);
		std::fprintf(ref_trace, "S %d %d %d %d", (int)(unsigned char)p.phase, (int)p.gyro_is_set, (int)p.acc_1_is_set,
		             (int)p.mag_1_is_set);
		put3t(p.gyro, p.time_gyro);
		put3t(p.acc_0, p.time_acc_0);
		put3t(p.acc_1, p.time_acc_1);
		put3t(p.mag_0, p.time_mag_0);
		put3t(p.mag_1, p.time_mag_1);
		std::fprintf(ref_trace, " %d %d %d %d %d %d %d\n", p.acc_count, p.mag_count, p.gyr_count, (int)p.Acc_initialized,
		             (int)p.Mag_initialized, (int)p.Gyr_initialized, (int)p.Kalman_initialized);
	}
	std::fprintf(ref_trace, "E");
	put3(p.avg_acc);
	put3(p.avg_mag);
	put3(p.avg_gyr);
	put3(p.variance_acc);
	put3(p.variance_mag);
	put3(p.variance_gyr);
	std::fprintf(ref_trace, " %d %d %d %d\n", (int)p.Acc_initialized, (int)p.Mag_initialized, (int)p.Gyr_initialized,
	             (int)p.Kalman_initialized);
	std::free(buf);
	return std::fclose(ref_trace) ? 1 : 0;
}
