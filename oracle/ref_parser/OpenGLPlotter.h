// Stand-in for the reference's GLFW plotter: the three members Parser.cpp calls, doing nothing.
#pragma once

class OpenGLPlotter
{
public:
	void Init() {}
	void run() {}
	void setMVPmatrix(double *) {}
};
