// taudem_amd_shim.cpp - the reference-side binding of INTEGRATION.md section 1, as a buildable file.
//
// Link the UNMODIFIED reference mains (src/PitRemovemn.cpp, src/D8FlowDirmn.cpp, src/aread8mn.cpp, src/DinfFlowDirmn.cpp,
// src/areadinfmn.cpp, src/DinfDecayAccummn.cpp, src/gridnetmn.cpp, src/Thresholdmn.cpp, src/D8FlowPathExtremeUpmn.cpp) against
// this file and -ltaudem_amd instead of flood.cpp / d8.cpp / aread8.cpp / ... + commonLib.cpp + tiffIO.cpp: every tool function the
// mains call (prototypes: src/flood.h:1-2, src/d8.h:5, src/aread8.h:3, src/tardemlib.h:70, src/areadinf.h:2,
// src/dinfdecayaccum.cpp:61-62, src/gridnet.cpp:54-55, src/Threshold.cpp:49, src/D8flowpathextremeup.cpp:58,
// src/DinfUpDependence.cpp:52, src/DinfRevAccum.cpp:51, src/DinfDistDown.cpp:66-67, src/DinfDistUp.cpp:65-66,
// src/D8HDistToStrm.cpp:57, src/gagewatershed.cpp:56, src/flowdircond.cpp:54, src/D8VDistToStrm.cpp:58, src/SlopeAveDown.cpp:59, src/retlimro.h, src/DinfAvalanche.cpp:62-63, src/CatchHydroGeo.cpp:69, src/InunDepth.h, src/DropAnalysis.h, src/PeukerDouglasmn.cpp:51, src/SinmapSI.cpp:138) forwards to the
// file-level C ABI, and nameadd() (src/commonLib.cpp:53-73, the only other symbol the mains use) is provided here.  No MPI and
// no GDAL at link time (their headers are only needed to COMPILE the mains, which include commonLib.h).
// oracle/Makefile builds oracle/_ref/shim_<tool> this way; tests/test_gpu_cli.py runs them against the reference's rasters.
#include <cstring>

#include "taudem_amd.h"

int flood(char* demfile, char* felfile, char* sfdrfile, int usesfdr, bool verbose, bool is_4Point, bool use_mask, char* maskfile)
{ return tdx_tool_pitremove(demfile, felfile, sfdrfile, usesfdr, verbose, is_4Point, use_mask, maskfile); }
int setdird8(char* demfile, char* pointfile, char* slopefile, char* flowfile, int useflowfile)
{ return tdx_tool_d8flowdir(demfile, pointfile, slopefile, flowfile, useflowfile); }
int aread8(char* pfile, char* afile, char* datasrc, char* lyrname, int uselyrname, int lyrno, char* wfile, int useOutlets, int usew, int contcheck)
{ return tdx_tool_aread8(pfile, afile, datasrc, lyrname, uselyrname, lyrno, wfile, useOutlets, usew, contcheck); }
int setdir(char* demfile, char* angfile, char* slopefile, char* flowfile, int useflowfile)
{ return tdx_tool_dinfflowdir(demfile, angfile, slopefile, flowfile, useflowfile); }
int area(char* angfile, char* scafile, char* datasrc, char* lyrname, int uselyrname, int lyrno, char* wfile, int useOutlets, int usew, int contcheck)
{ return tdx_tool_areadinf(angfile, scafile, datasrc, lyrname, uselyrname, lyrno, wfile, useOutlets, usew, contcheck); }
int dmarea(char* angfile, char* adecfile, char* dmfile, char* datasrc, char* lyrname, int uselyrname, int lyrno, char* wfile, int useOutlets, int usew, int contcheck)
{ return tdx_tool_dinfdecayaccum(angfile, adecfile, dmfile, datasrc, lyrname, uselyrname, lyrno, wfile, useOutlets, usew, contcheck); }
int gridnet(char* pfile, char* plenfile, char* tlenfile, char* gordfile, char* maskfile, char* datasrc, char* lyrname, int uselyrname, int lyrno, int useMask, int useOutlets, int thresh)
{ return tdx_tool_gridnet(pfile, plenfile, tlenfile, gordfile, maskfile, datasrc, lyrname, uselyrname, lyrno, useMask, useOutlets, thresh); }
int d8flowpathextremeup(char* pfile, char* safile, char* ssafile, int usemax, char* datasrc, char* lyrname, int uselyrname, int lyrno, int useOutlets, int contcheck)
{ return tdx_tool_d8flowpathextremeup(pfile, safile, ssafile, usemax, datasrc, lyrname, uselyrname, lyrno, useOutlets, contcheck); }
int depgrd(char* angfile, char* dgfile, char* depfile)
{ return tdx_tool_dinfupdependence(angfile, dgfile, depfile); }
int dsaccum(char* angfile, char* wgfile, char* raccfile, char* dmaxfile)
{ return tdx_tool_dinfrevaccum(angfile, wgfile, raccfile, dmaxfile); }
int dinfdistdown(char* angfile, char* felfile, char* slpfile, char* wfile, char* srcfile, char* dtsfile, int statmethod, int typemethod, int usew, int concheck)
{ return tdx_tool_dinfdistdown(angfile, felfile, slpfile, wfile, srcfile, dtsfile, statmethod, typemethod, usew, concheck); }
int dinfdistup(char* angfile, char* felfile, char* slpfile, char* wfile, char* rtrfile, int statmethod, int typemethod, int usew, int concheck, float thresh)
{ return tdx_tool_dinfdistup(angfile, felfile, slpfile, wfile, rtrfile, statmethod, typemethod, usew, concheck, thresh); }
int retlimro(char* angfile, char* wgfile, char* rcfile, char* qrlfile)
{ return tdx_tool_retlimflow(angfile, wgfile, rcfile, qrlfile); }
int avalancherunoutgrd(char* angfile, char* felfile, char* assfile, char* rzfile, char* dmfile, float thresh, float alpha, int path)
{ return tdx_tool_dinfavalanche(angfile, felfile, assfile, rzfile, dmfile, thresh, alpha, path); }
int distgrid(char* pfile, char* srcfile, char* distfile, int thresh)
{ return tdx_tool_d8hdisttostrm(pfile, srcfile, distfile, thresh); }
int gagewatershed(char* pfile, char* wfile, char* datasrc, char* lyrname, int uselyrname, int lyrno, char* idfile, int writeid, int writeupid, char* upidfile)
{ return tdx_tool_gagewatershed(pfile, wfile, datasrc, lyrname, uselyrname, lyrno, idfile, writeid, writeupid, upidfile); }
int flowdircond(char* pfile, char* zfile, char* zfdcfile)
{ return tdx_tool_flowdircond(pfile, zfile, zfdcfile); }
int d8vdistdown(char* pfile, char* felfile, char* srcfile, char* distfile, int thresh)
{ return tdx_tool_d8vdisttostrm(pfile, felfile, srcfile, distfile, thresh); }
int sloped(char* pfile, char* felfile, char* slpdfile, double dn)
{ return tdx_tool_slopeavedown(pfile, felfile, slpdfile, dn); }
int dsllArea(char* angfile, char* ctptfile, char* dmfile, char* datasrc, char* lyrname, int uselyrname, int lyrno, char* qfile, char* dgfile, int useOutlets, int contcheck, float cSol)
{ return tdx_tool_dinfconclimaccum(angfile, ctptfile, dmfile, datasrc, lyrname, uselyrname, lyrno, qfile, dgfile, useOutlets, contcheck, cSol); }
int tlaccum(char* angfile, char* tsupfile, char* tcfile, char* tlafile, char* depfile, char* cinfile, char* coutfile, char* datasrc, char* lyrname, int uselyrname, int lyrno, int useOutlets, int usec, int contcheck)
{ return tdx_tool_dinftranslimaccum(angfile, tsupfile, tcfile, tlafile, depfile, cinfile, coutfile, datasrc, lyrname, uselyrname, lyrno, useOutlets, usec, contcheck); }
int catchhydrogeo(char* handfile, char* catchfile, char* catchlistfile, char* slpfile, char* hfile, char* hpfile)
{ return tdx_tool_catchhydrogeo(handfile, catchfile, catchlistfile, slpfile, hfile, hpfile); }
int inundepth(char* handfile, char* catchfile, char* maskfile, char* fcfile, char* hpfile, char* mapfile, char* depthfile)
{ return tdx_tool_inundepth(handfile, catchfile, maskfile, fcfile, hpfile, mapfile, depthfile); }
int dropan(char* areafile, char* dirfile, char* elevfile, char* ssafile, char* dropfile, char* datasrc, char* lyrname, int uselyrname, int lyrno, float threshmin, float threshmax, int nthresh, int steptype, float* threshopt)
{ return tdx_tool_dropanalysis(areafile, dirfile, elevfile, ssafile, dropfile, datasrc, lyrname, uselyrname, lyrno, threshmin, threshmax, nthresh, steptype, threshopt); }
int peukerdouglas(char* felfile, char* ssfile, float* p)
{ return tdx_tool_peukerdouglas(felfile, ssfile, p); }
int sindexcombined(char* slopefile, char* scaterrainfile, char* scarminroadfile, char* scarmaxroadfile, char* tergridfile, char* terparfile, char* satfile, char* sincombinedfile, double Rminter, double Rmaxter, double* par)
{ return tdx_tool_sinmapsi(slopefile, scaterrainfile, scarminroadfile, scarmaxroadfile, tergridfile, terparfile, satfile, sincombinedfile, Rminter, Rmaxter, par); }
int twigrid(char* slopefile, char* areafile, char* twifile)
{ return tdx_tool_twi(slopefile, areafile, twifile); }
int slopearea(char* slopefile, char* scafile, char* safile, float* p)
{ return tdx_tool_slopearea(slopefile, scafile, safile, p); }
int atanbgrid(char* slopefile, char* areafile, char* atanbfile)
{ return tdx_tool_slopearearatio(slopefile, areafile, atanbfile); }
int lengtharea(char* plenfile, char* ad8file, char* ssfile, float* p)
{ return tdx_tool_lengtharea(plenfile, ad8file, ssfile, p); }
int setregion(char* fdrfile, char* regiongwfile, char* newfile, int32_t regionID)
{ return tdx_tool_setregion(fdrfile, regiongwfile, newfile, regionID); }
int editraster(char* rasterfile, char* newfile, char* changefile)
{ return tdx_tool_editraster(rasterfile, newfile, changefile); }
int threshold(char* ssafile, char* srcfile, char* maskfile, float thresh, int usemask)
{ return tdx_tool_threshold(ssafile, srcfile, maskfile, thresh, usemask); }

// nameadd(full, arg, suff): `suff` goes in front of the extension of `arg` (the last '.'; none: appended); a suffix that
// brings its own extension replaces the original one.  Same contract as src/commonLib.cpp:53-73.
int nameadd(char* full, char* arg, const char* suff) {
    const char* dot = strrchr(arg, '.');
    const size_t stem = dot ? size_t(dot - arg) : strlen(arg);
    memcpy(full, arg, stem);
    full[stem] = '\0';
    strcat(full, suff);
    if (dot && !strrchr(suff, '.')) strcat(full, dot);
    return int(stem);   // the reference returns the length of the stem
}
