// check.h — the assertions of the stand-alone *_check.cpp programs (built and run by tests/hostcheck.py).
//   CHECK(x);                      a failed check reports its file, line and expression and the program goes on
//   CHECK(cond, "fmt", args...);   the same with a printf-style explanation
//   g_where = "which case";        optional: named in the reports that follow
//   return check_finish("... ok"); at the end of main: prints the ok line only when nothing failed, and gives the exit status
// Reports go to stderr (unbuffered: they survive a crash further on), at most 40 of them; the ok line goes to stdout.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <string>

inline long g_checks = 0, g_failed = 0;
inline std::string g_where;

__attribute__((format(printf, 4, 5))) inline void check_failed(const char* file, int line, const char* expr, const char* fmt, ...) {
    if (g_failed++ >= 40) return;
    fprintf(stderr, "FAILED %s:%d%s%s%s: %s", file, line, g_where.empty() ? "" : " [", g_where.c_str(), g_where.empty() ? "" : "]", expr);
    if (fmt) {
        va_list ap;
        va_start(ap, fmt);
        fprintf(stderr, ": ");
        vfprintf(stderr, fmt, ap);
        va_end(ap);
    }
    fprintf(stderr, "\n");
}
inline void check_failed(const char* file, int line, const char* expr) { check_failed(file, line, expr, nullptr); }

#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        g_checks++;                                                             \
        if (!(cond)) check_failed(__FILE__, __LINE__, #cond, ##__VA_ARGS__);    \
    } while (0)

inline int check_finish(const char* ok) {
    if (g_failed) {
        fprintf(stderr, "%ld of %ld checks failed\n", g_failed, g_checks);
        return 1;
    }
    printf("%s (%ld checks)\n", ok, g_checks);
    return 0;
}
