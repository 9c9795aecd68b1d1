// Stand-in for the reference server's Winsock header, so that its Parser.cpp builds on Linux
// (oracle/Makefile stages this file next to a copy of Parser.cpp under oracle/_ref/).  It carries the
// standard headers Parser.cpp gets through the real one and the members Parser::run calls; the driver
// never calls run, so they do nothing.
#pragma once
#include <array>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <iostream>
#include <mutex>
#include <regex>
#include <string>
#include <thread>
#include <vector>

extern FILE *ref_trace;  // driver.cpp: where the stubs record what the parser hands them

class Server
{
public:
	std::condition_variable *getCV() { return nullptr; }
	std::vector<std::string> getSensorReadings() { return {}; }
	void clearSensorReadings() {}
	bool getLoop() { return false; }
};
