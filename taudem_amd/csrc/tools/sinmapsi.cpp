// sinmapsi slp sca calpar cal si sat rminter rmaxter g rhow [scamin scamax]
// sinmapsi -slp slp -sca sca -calpar calpar -cal cal -si si -sat sat -par rminter rmaxter g rhow [-scamin scamin] [-scamax scamax]
// (argument surface of src/SinmapSImn.cpp:50-249: 10 positional arguments, 12 positional arguments, or flags when there are more than 12 words)
#include "cli_common.hpp"

static int usage(const char* prog) {
    printf("Simple Use:\n %s <basefilename>\n", prog);
    printf("Use with specific file names:\n %s -slp <slopefile>\n", prog);
    printf("-sca <scafile> -calpar <calpfile> -cal <calfile> -si <sifile> -sat <satfile> -par <rminter> <rmaxter> <g> <rhow> [-scamin <scaminfile> -scamax <scamaxfile>] \n");
    printf("<basefilename> is the name of the base digital elevation model without suffixes for simple input. Suffixes 'slp', 'sca' and 'sa' will be appended. \n");
    printf("<slopefile> is the name of the input slope file.\n");
    printf("<scafile> is the name of input contributing area file.\n");
    printf("<calpfile> is the name of input calibration region parameter text file.\n");
    printf("<calfile> is the name of input calibration grid file file.\n");
    printf("<sifile> is the name of output combined stability index grid file.\n");
    printf("<satfile> is the name of output <TODO> file.\n");
    printf("<rminter> is the minimum terrain recharge constant.\n");
    printf("<rmaxter> is the maximum terrain recharge constant.\n");
    printf("<g> is the gravitational force.\n");
    printf("<rhow> is the <TODO> constant.\n");
    printf("<scaminfile> is the name of input minimum contributing area file.\n");
    printf("<scamaxfile> is the name of input maximum contributing area file.\n");
    return 0;
}

int main(int argc, char** argv) {
    cli::take_gpus(argc, argv);
    std::string slp, sca, scamin, scamax, cal, calpar, sat, si;
    float rminter = 0.0f, rmaxter = 0.0f, tpar[2] = {0.0f, 0.0f};   // scanned as floats, widened for the call
    if (argc < 11) return usage(argv[0]);
    if (argc == 11 || argc == 13) {
        slp = argv[1]; sca = argv[2]; calpar = argv[3]; cal = argv[4]; si = argv[5]; sat = argv[6];
        sscanf(argv[7], "%f", &rminter);
        sscanf(argv[8], "%f", &rmaxter);
        sscanf(argv[9], "%f", &tpar[0]);
        sscanf(argv[10], "%f", &tpar[1]);
        if (argc == 13) { scamin = argv[11]; scamax = argv[12]; }
    } else if (argc > 13) {
        cli::Args a(argc, argv);
        while (a.more()) {
            if (a.is("-slp")) { if (!a.value(slp)) return usage(argv[0]); }
            else if (a.is("-sca")) { if (!a.value(sca)) return usage(argv[0]); }
            else if (a.is("-scamin")) { if (!a.value(scamin)) return usage(argv[0]); }
            else if (a.is("-scamax")) { if (!a.value(scamax)) return usage(argv[0]); }
            else if (a.is("-cal")) { if (!a.value(cal)) return usage(argv[0]); }
            else if (a.is("-calpar")) { if (!a.value(calpar)) return usage(argv[0]); }
            else if (a.is("-si")) { if (!a.value(si)) return usage(argv[0]); }
            else if (a.is("-sat")) { if (!a.value(sat)) return usage(argv[0]); }
            else if (a.is("-par")) {
                if (a.argc <= a.i + 4) return usage(argv[0]);
                sscanf(a.argv[a.i + 1], "%f", &rminter);
                sscanf(a.argv[a.i + 2], "%f", &rmaxter);
                sscanf(a.argv[a.i + 3], "%f", &tpar[0]);
                sscanf(a.argv[a.i + 4], "%f", &tpar[1]);
                a.i += 5;
            }
            else return usage(argv[0]);
        }
    } else return usage(argv[0]);   // 11 arguments: the reference goes on with file names it never set
    const double par[2] = {double(tpar[0]), double(tpar[1])};
    const int err = tdx_tool_sinmapsi(slp.c_str(), sca.c_str(), scamin.c_str(), scamax.c_str(), cal.c_str(), calpar.c_str(), sat.c_str(), si.c_str(), double(rminter),
                                      double(rmaxter), par);
    if (err != 0 && !cli::is_abort_code(err)) { printf("Sinmap Stability Index Error %d\n", err); return 0; }
    return cli::finish("Sinmap Stability Index", err);
}
